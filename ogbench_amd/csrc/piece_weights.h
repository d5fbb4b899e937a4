// piece_weights.h -- the integer weights of an active-edge set (plain C++, no
// device builtins: tests/test_piece_weights_cpu.py compiles it without HIP).
//
// Per contact slot s with edge activities a0 (n+t), a1 (n-t), a2 (n), each 0
// or 1:  T = a0 + a1,  D = a0 - a1,  S = T + 2 a2  (point_contact.h states the
// normal equations they weight).  Two builders, the same values:
//   * piece_weights(A, p): from the integer mask A (bits 3s, 3s+1, 3s+2), by
//     integer arithmetic and a conversion -- the definition;
//   * piece_weights_from(e, p): from the activities as doubles (0.0 or 1.0,
//     edge_on of the comparison that decides each edge), by adds and one fma.
//     Every value is an integer of magnitude <= 4, so each operation is exact
//     and the result is the definition's, bit for bit.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define OGBX_PW_FN __host__ __device__ inline
#else
#define OGBX_PW_FN inline
#endif

namespace ogbx {

// A2 = a0 + a1 + a2 and C2 = a2 of slot 2 feed the lean loop's double-angle
// form of the corner terms (local_piece_min).
// (S3, T3, D3: the fourth slot of the kG = 4 generic evaluation.)
struct PieceWeights {
  double S0, T0, D0, S1, T1, D1, S2, T2, D2, A2, C2, S3, T3, D3;
};

template <int kG = 3>
OGBX_PW_FN void piece_weights(uint32_t A, PieceWeights& p) {
  auto one = [&](int s, double& S, double& T, double& D) {
    const int a0 = (A >> (3 * s)) & 1, a1 = (A >> (3 * s + 1)) & 1, a2 = (A >> (3 * s + 2)) & 1;
    T = (double)(a0 + a1);
    D = (double)(a0 - a1);
    S = (double)(a0 + a1 + 2 * a2);
  };
  one(0, p.S0, p.T0, p.D0);
  one(1, p.S1, p.T1, p.D1);
  one(2, p.S2, p.T2, p.D2);
  if (kG > 3) one(3, p.S3, p.T3, p.D3);
  const int a2 = (A >> 8) & 1;
  p.A2 = (double)(((A >> 6) & 1) + ((A >> 7) & 1) + a2);
  p.C2 = (double)a2;
}

// The activities of the nine edges of slots 0..2 as doubles, in mask-bit order.
struct EdgeActs {
  double a[9];
};

// One select on the high word: 1.0 and 0.0 share their (zero) low word.
OGBX_PW_FN double edge_on(bool active) { return active ? 1.0 : 0.0; }

// Slots 0..2 (S3, T3, D3 are left alone: the lean loop has three slots).
OGBX_PW_FN void piece_weights_from(const EdgeActs& e, PieceWeights& p) {
  auto one = [](const double* a, double& S, double& T, double& D) {
    T = a[0] + a[1];
    D = a[0] - a[1];
    S = __builtin_fma(2.0, a[2], T);
  };
  one(e.a + 0, p.S0, p.T0, p.D0);
  one(e.a + 3, p.S1, p.T1, p.D1);
  one(e.a + 6, p.S2, p.T2, p.D2);
  p.A2 = p.T2 + e.a[8];
  p.C2 = e.a[8];
}

}  // namespace ogbx
