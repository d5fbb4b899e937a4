// framestack.hip -- frame stacks of batched env observations (include/ogbx_framestack.h):
// FrameStackWrapper of impls/utils/env_utils.py:48-76 for every env in one launch.
//
// A stack is n x P x k x E bytes.  Seen as byte streams, `next` is `prev`
// shifted by E bytes with the last E bytes of every k*E-byte pixel replaced
// from `obs`.  A lane owns one 16-byte unit of the output (the stacks start on
// 16-byte boundaries, so every unit is one aligned dwordx4 store):
//   fast path  no env the unit touches is done: one 16-byte load of
//              prev + g + E at its natural (any) byte alignment and per dword
//              one dword load of obs, merged under a byte mask; all five loads
//              are unconditional, so they are in flight together.  Needs
//              (k-1)*E >= 3, so that a dword meets at most one obs slot, and
//              rows of 16 bytes or more.  A done env's final stack is the
//              same compose from final_obs.
//   byte path  everything else (units that span two envs, the ends of the
//              buffers, done envs' k copies, fill, k == 1, (k-1)*E < 3): the
//              16 bytes are gathered one by one, the position (env, pixel,
//              slot) stepped along, and stored as one unit when all are
//              valid, bytewise otherwise.
// No lane reads a byte another lane writes (out of place), there is no LDS and
// no barrier.  Offsets are 32-bit when every byte count stays below 2^31 and
// 64-bit otherwise (two instances).
#include "../../include/ogbx_framestack.h"

#include "common.h"

namespace ogbx {
namespace {

struct FsPtrs {
  const uint8_t* obs;
  const uint8_t* prev;
  const uint8_t* m0;  // push: terminated; fill: mask
  const uint8_t* m1;  // push: truncated
  const uint8_t* final_obs;
  uint8_t* next;  // fill: stack
  uint8_t* final_stack;
};

template <typename Idx>
struct FsDims {
  Idx n;          // envs
  Idx total;      // bytes of a stack, n * row
  Idx row;        // bytes of one env's stack, P * k * E
  Idx obs_row;    // bytes of one env's frame, P * E
  Idx obs_total;  // n * obs_row
  Idx E;
  Idx kE;
  Idx hist;  // (k - 1) * E: a pixel's bytes that come from prev
};

__device__ __forceinline__ uint4 fs_load16(const uint8_t* p) {  // any byte alignment
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

__device__ __forceinline__ uint32_t fs_load4(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

template <bool FILL, typename Idx>
__device__ __forceinline__ bool fs_done(const FsPtrs& a, Idx e) {
  if (FILL) return a.m0 ? a.m0[e] != 0 : true;
  bool d = false;
  if (a.m0) d = a.m0[e] != 0;
  if (a.m1) d = d | (a.m1[e] != 0);
  return d;
}

// 16 bytes at the 16-byte aligned dst: one store when all are valid
__device__ __forceinline__ void fs_put16(uint8_t* dst, const uint32_t (&w)[4], uint32_t valid) {
  if (valid == 0xffffu) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    return;
  }
#pragma unroll
  for (int b = 0; b < 16; ++b)
    if (valid >> b & 1u) dst[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
}

template <typename Idx, bool FILL>
__global__ void __launch_bounds__(256) framestack_kernel(FsPtrs a, FsDims<Idx> s, Idx n_units, int fast) {
  const Idx u = (Idx)blockIdx.x * 256 + threadIdx.x;
  if (u >= n_units) return;
  const Idx g = u * 16;  // byte offset of the unit in the stack
  Idx e = g / s.row;
  Idx j = g - e * s.row;  // ... in the env's row
  const Idx p = j / s.kE;
  Idx q = j - p * s.kE;                // ... in the pixel
  Idx ob = e * s.obs_row + p * s.E;    // the pixel's frame bytes in obs
  // the done flags of the one or two envs the unit touches (the fast path needs
  // row >= 16): the loads are issued here, ahead of the unit's own, and first
  // used behind them; the host passes both masks or none (a NULL one is
  // replaced by the other)
  const bool span = j + 16 > s.row;
  const Idx e2 = (span && e + 1 < s.n) ? e + 1 : e;
  uint32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  if (!FILL && a.m0) {
    x0 = a.m0[e], x1 = a.m1[e];
    y0 = a.m0[e2], y1 = a.m1[e2];
  }
  bool want_final = !FILL && a.final_stack != nullptr;

  // Fast path.  The compose itself does not see env boundaries (an env ends
  // where a slot ends, and obs is contiguous across envs); only the done flags
  // of the one or two envs the unit touches (row >= 16) decide.  Its loads are
  // unconditional and issued together: the unit of prev at g + E, and per
  // dword the dword of obs that holds its slot bytes (the pixel's own address
  // under an empty mask when it has none).  ob >= 4 and ob + 2 E + 11 <=
  // obs_total keep every such dword inside obs: a dword with slot bytes of the
  // pixel at oo starts after oo - 4 and ends by oo + E + 3, and oo <= ob + E + 8.
  if (!FILL && fast && g + s.E + 16 <= s.total && ob >= 4 && ob + 2 * s.E + 11 <= s.obs_total) {
    const uint4 v = fs_load16(a.prev + g + s.E);
    Idx at[4];
    uint32_t m[4], ow[4];
    Idx qq = q, oo = ob;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool touches = qq + 4 > s.hist;  // bytes [lo, hi) of the dword are slot bytes of pixel oo
      const uint32_t lo = qq >= s.hist ? 0u : (uint32_t)(s.hist - qq) & 3u;
      const Idx left = s.kE - qq;
      const uint32_t hi = left < 4 ? (uint32_t)left : 4u;
      m[c] = touches ? (0xffffffffu >> (32u - 8u * hi)) & (0xffffffffu << (8u * lo)) : 0u;
      at[c] = touches ? oo + qq - s.hist : oo;  // dword byte b is obs[at + b]
      ow[c] = fs_load4(a.obs + at[c]);
      qq += 4;
      if (qq >= s.kE) {
        qq -= s.kE;
        oo += s.E;
      }
    }
    // keeps the flags' first use (and so their wait) behind the loads above
    asm volatile("" : "+v"(x0), "+v"(x1), "+v"(y0), "+v"(y1));
    if ((x0 | x1 | y0 | y1) == 0) {
      *reinterpret_cast<uint4*>(a.next + g) = make_uint4((v.x & ~m[0]) | (ow[0] & m[0]), (v.y & ~m[1]) | (ow[1] & m[1]),
                                                         (v.z & ~m[2]) | (ow[2] & m[2]), (v.w & ~m[3]) | (ow[3] & m[3]));
      return;
    }
    if (!span && want_final) {  // d: the stack the episode ended with; `next` is k copies of obs, below
#pragma unroll
      for (int c = 0; c < 4; ++c) ow[c] = fs_load4(a.final_obs + at[c]);
      *reinterpret_cast<uint4*>(a.final_stack + g) =
          make_uint4((v.x & ~m[0]) | (ow[0] & m[0]), (v.y & ~m[1]) | (ow[1] & m[1]), (v.z & ~m[2]) | (ow[2] & m[2]),
                     (v.w & ~m[3]) | (ow[3] & m[3]));
      want_final = false;
    }
  }
  bool d = FILL ? fs_done<true>(a, e) : (x0 | x1) != 0;

  uint32_t nw[4] = {0, 0, 0, 0}, fw[4] = {0, 0, 0, 0};
  uint32_t nvalid = 0, fvalid = 0;
  Idx r = q % s.E;  // ... in the slot
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    if (g + b < s.total) {
      const bool in_slot = q >= s.hist;
      const Idx oi = ob + r;
      uint32_t nb = 0;
      if (FILL) {
        if (d) {
          nb = a.obs[oi];
          nvalid |= 1u << b;
        }
      } else {
        // q < hist puts g + b + E inside the same pixel
        const uint32_t hv = (in_slot || (d && !want_final)) ? 0u : (uint32_t)a.prev[g + b + s.E];
        if (d) {
          nb = a.obs[oi];
          if (want_final) {
            const uint32_t fb = in_slot ? (uint32_t)a.final_obs[oi] : hv;
            fw[b >> 2] |= fb << (8 * (b & 3));
            fvalid |= 1u << b;
          }
        } else {
          nb = in_slot ? (uint32_t)a.obs[oi] : hv;
        }
        nvalid |= 1u << b;
      }
      nw[b >> 2] |= nb << (8 * (b & 3));
    }
    ++j, ++q, ++r;
    if (r == s.E) r = 0;
    if (q == s.kE) {
      q = 0;
      ob += s.E;  // pixel P of env e is pixel 0 of env e + 1
    }
    if (j == s.row) {
      j = 0;
      ++e;
      d = e < s.n ? fs_done<FILL>(a, e) : false;
    }
  }
  fs_put16(a.next + g, nw, nvalid);
  if (!FILL && fvalid) fs_put16(a.final_stack + g, fw, fvalid);
}

struct FsSizes {
  int64_t n, E, kE, hist, obs_row, row, obs_total, total;
};

ogbx_status fs_sizes(const std::string& who, const ogbx_framestack_shape* sh, FsSizes* z) {
  OGBX_CHECK(sh, OGBX_EINVAL, who + "null shape");
  OGBX_CHECK(sh->n >= 0, OGBX_EINVAL, who + "n must be >= 0");
  OGBX_CHECK(sh->pixels >= 1, OGBX_EINVAL, who + "pixels must be >= 1");
  OGBX_CHECK(sh->elem_bytes >= 1, OGBX_EINVAL, who + "elem_bytes must be >= 1");
  OGBX_CHECK(sh->num_stack >= 1, OGBX_EINVAL, who + "num_stack must be >= 1");
  z->n = sh->n;
  z->E = sh->elem_bytes;
  int64_t padded = 0;
  const bool over = __builtin_mul_overflow(z->E, (int64_t)sh->num_stack, &z->kE) ||
                    __builtin_mul_overflow(sh->pixels, z->E, &z->obs_row) ||
                    __builtin_mul_overflow(sh->pixels, z->kE, &z->row) ||
                    __builtin_mul_overflow(z->n, z->obs_row, &z->obs_total) ||
                    __builtin_mul_overflow(z->n, z->row, &z->total) ||
                    __builtin_add_overflow(z->total, z->kE, &padded) || __builtin_add_overflow(padded, 64, &padded);
  OGBX_CHECK(!over, OGBX_EINVAL, who + "the byte counts do not fit int64");
  // one lane per 16 bytes, 256 lanes per block
  OGBX_CHECK(z->total / 4096 < (1ll << 31) - 1, OGBX_EINVAL, who + "the stack is too large for one launch");
  z->hist = z->kE - z->E;
  return OGBX_OK;
}

struct FsRange {
  const void* p;
  int64_t bytes;
  const char* name;
};

bool fs_overlap(const FsRange& x, const FsRange& y) {
  if (!x.p || !y.p || x.bytes <= 0 || y.bytes <= 0) return false;
  const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
  return a < b + (uintptr_t)y.bytes && b < a + (uintptr_t)x.bytes;
}

// No output range may meet an input range or another output.
ogbx_status fs_disjoint(const std::string& who, std::initializer_list<FsRange> outs,
                        std::initializer_list<FsRange> ins) {
  for (const FsRange& o : outs) {
    for (const FsRange& i : ins)
      OGBX_CHECK(!fs_overlap(o, i), OGBX_EINVAL, who + o.name + " overlaps " + i.name);
    for (const FsRange& o2 : outs)
      OGBX_CHECK(&o == &o2 || !fs_overlap(o, o2), OGBX_EINVAL, who + o.name + " overlaps " + o2.name);
  }
  return OGBX_OK;
}

ogbx_status fs_device(const std::string& who, std::initializer_list<FsRange> ptrs) {
  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  for (const FsRange& r : ptrs)
    OGBX_CHECK(!r.p || on_device(r.p, dev), OGBX_EINVAL,
               who + r.name + " is not memory of the current device");
  return OGBX_OK;
}

template <typename Idx, bool FILL>
ogbx_status fs_launch_as(const FsPtrs& a, const FsSizes& z, hipStream_t stream) {
  FsDims<Idx> s;
  s.n = (Idx)z.n, s.total = (Idx)z.total, s.row = (Idx)z.row, s.obs_row = (Idx)z.obs_row;
  s.obs_total = (Idx)z.obs_total, s.E = (Idx)z.E, s.kE = (Idx)z.kE, s.hist = (Idx)z.hist;
  const int64_t units = (z.total + 15) / 16;
  const int64_t blocks = (units + 255) / 256;
  const int fast = !FILL && z.hist >= 3 && z.row >= 16;
  hipLaunchKernelGGL((framestack_kernel<Idx, FILL>), dim3((uint32_t)blocks), dim3(256), 0, stream, a, s, (Idx)units,
                     fast);
  OGBX_LAUNCHED(FILL ? "framestack fill launch" : "framestack push launch");
  return OGBX_OK;
}

template <bool FILL>
ogbx_status fs_launch(const FsPtrs& a, const FsSizes& z, void* stream) {
  // 32-bit offsets while every sum the kernel forms (at most total + kE + 16) stays below 2^31
  if (z.total + z.kE + 64 < (1ll << 31)) return fs_launch_as<uint32_t, FILL>(a, z, (hipStream_t)stream);
  return fs_launch_as<uint64_t, FILL>(a, z, (hipStream_t)stream);
}

}  // namespace
}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_framestack_abi_version(void) { return OGBX_FRAMESTACK_ABI_VERSION; }

ogbx_status ogbx_framestack_fill(const ogbx_framestack_shape* shape, const void* obs, const uint8_t* mask,
                                 void* stack, void* stream) {
  const std::string who = "ogbx_framestack_fill: ";
  FsSizes z;
  if (ogbx_status st = fs_sizes(who, shape, &z)) return st;
  OGBX_CHECK(obs && stack, OGBX_EINVAL, who + "null obs or stack");
  OGBX_CHECK(((uintptr_t)stack & 15) == 0, OGBX_EINVAL, who + "stack must start on a 16-byte boundary");
  const FsRange out{stack, z.total, "stack"};
  const FsRange in_obs{obs, z.obs_total, "obs"}, in_mask{mask, z.n, "mask"};
  if (ogbx_status st = fs_disjoint(who, {out}, {in_obs, in_mask})) return st;
  if (z.n == 0) return OGBX_OK;
  if (ogbx_status st = fs_device(who, {out, in_obs, in_mask})) return st;
  FsPtrs a{};
  a.obs = (const uint8_t*)obs, a.m0 = mask, a.next = (uint8_t*)stack;
  return fs_launch<true>(a, z, stream);
}

ogbx_status ogbx_framestack_push(const ogbx_framestack_shape* shape, const void* obs, const void* prev,
                                 const uint8_t* terminated, const uint8_t* truncated, const void* final_obs,
                                 void* next, void* final_stack, void* stream) {
  const std::string who = "ogbx_framestack_push: ";
  FsSizes z;
  if (ogbx_status st = fs_sizes(who, shape, &z)) return st;
  OGBX_CHECK(obs && prev && next, OGBX_EINVAL, who + "null obs, prev or next");
  OGBX_CHECK(!final_stack || final_obs, OGBX_EINVAL, who + "final_stack needs final_obs");
  OGBX_CHECK(!final_stack || terminated || truncated, OGBX_EINVAL,
             who + "final_stack needs a terminated or truncated mask");
  OGBX_CHECK((((uintptr_t)prev | (uintptr_t)next | (uintptr_t)final_stack) & 15) == 0, OGBX_EINVAL,
             who + "prev, next and final_stack must start on a 16-byte boundary");
  const FsRange o_next{next, z.total, "next"}, o_final{final_stack, z.total, "final_stack"};
  const FsRange i_obs{obs, z.obs_total, "obs"}, i_prev{prev, z.total, "prev"}, i_term{terminated, z.n, "terminated"},
      i_trunc{truncated, z.n, "truncated"}, i_fobs{final_stack ? final_obs : nullptr, z.obs_total, "final_obs"};
  if (ogbx_status st = fs_disjoint(who, {o_next, o_final}, {i_obs, i_prev, i_term, i_trunc, i_fobs})) return st;
  if (z.n == 0) return OGBX_OK;
  if (ogbx_status st = fs_device(who, {o_next, o_final, i_obs, i_prev, i_term, i_trunc, i_fobs})) return st;
  FsPtrs a{};
  a.obs = (const uint8_t*)obs, a.prev = (const uint8_t*)prev;
  a.m0 = terminated ? terminated : truncated, a.m1 = truncated ? truncated : terminated;  // both or none
  a.final_obs = final_stack ? (const uint8_t*)final_obs : nullptr;
  a.next = (uint8_t*)next, a.final_stack = (uint8_t*)final_stack;
  return fs_launch<false>(a, z, stream);
}

}  // extern "C"
