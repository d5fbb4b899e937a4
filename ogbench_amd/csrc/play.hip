// play.hip -- powderworld play-data collection on gfx950 (include/ogbx_play.h):
// the open-loop action plan of the play policy in one launch, the batched
// random semantic action, and the C-ABI of the data-collection reset (whose
// kernels live with the other powder kernels, powder.hip).
//
// Reference (hliuson/ogbench):
//   collection loop                      data_gen_scripts/generate_powderworld.py:49-81
//   Fill / Line / Square behaviours      ogbench/powderworld/behaviors.py:34-115
//   sample_semantic_action               ogbench/powderworld/powderworld_env.py:446-451
//
// play_plan_kernel: one lane per env walks the T steps of its episode with the
// whole policy state in registers (behaviour kind, its reset draws, its step
// counter, the held semantic action) and writes actions[t, e] -- consecutive
// lanes write consecutive ints of a step's row.  No sequence is stored: entry i
// of a behaviour is a closed form of i and the reset draws.  A lane's draws are
// popped from a Philox stream whose counter is (global env, episode, pop
// index), or from the env's row of an injected tape.
#include <hip/hip_runtime.h>

#include "../../include/ogbx_play.h"
#include "common.h"
#include "powder_play.h"

namespace ogbx {

constexpr int kPlayThreads = 64;  // one wave per workgroup: N / 64 workgroups spread over the CUs
constexpr uint32_t kPlaySemanticSlot = 0x80000000u;

struct PlayArgs {
  ogbx_play_config cfg;
  int64_t n;
  int32_t T;
  int32_t* actions;
  const double* tape;
  int64_t tape_len;
  int64_t* short_count;
  ogbx_play_outputs out;
  uint32_t k0, k1;
};

// The env's source of draws: Philox pops, or the next values of its tape row.
struct PlayDraws {
  const double* tape;  // this env's row, or NULL
  int64_t tape_len;
  uint32_t c0, c1, c3, k0, k1;
  int32_t used;
  bool ran_out;

  __device__ __forceinline__ u32x4 words() {
    const u32x4 w = philox4x32_10({c0, c1, (uint32_t)used, c3}, k0, k1);
    used += 1;
    return w;
  }
  __device__ __forceinline__ double taped() {
    double v = 0.0;
    if ((int64_t)used < tape_len) v = tape[used];
    else ran_out = true;
    used += 1;
    return v;
  }
  __device__ __forceinline__ double uniform() {
    if (tape) return taped();
    const u32x4 w = words();
    return u01_from(w.x, w.y);
  }
  // integer in [lo, lo + n)
  __device__ __forceinline__ int integer(int lo, int n) {
    if (tape) {
      const double v = taped();
      const int i = v >= (double)(lo + n) ? lo + n - 1 : (v >= (double)lo ? (int)v : lo);  // NaN -> lo
      return i;
    }
    return lo + (int)bounded_u32(words().x, (uint32_t)n);
  }
};

// A behaviour after its reset draws (behaviors.py).  kind 0 Fill: a = flip_x,
// b = flip_y, swap = flip_xy.  1 Line: a = target, b = flip_dir, swap =
// flip_xy.  2 Square: a = x1, b = y1, len = length, rev = reverse bit of side s
// at bit s, perm = side of quarter q at bits 2q..2q+1.
struct PlayBehavior {
  int kind, elem, a, b, swap, len, rev, perm, step, count;

  __device__ __forceinline__ void choose(PlayDraws& d, const ogbx_play_config& c) {
    const double u = d.uniform();
    kind = (c.cdf[0] <= u ? 1 : 0) + (c.cdf[1] <= u ? 1 : 0);  // searchsorted(cdf, u, 'right'), cdf[2] = 1 > u
    const int size = c.size;
    elem = d.integer(0, c.num_elems);
    step = 0;
    swap = len = rev = perm = 0;
    if (kind == 0) {
      a = d.integer(0, 2);
      b = d.integer(0, 2);
      swap = d.integer(0, 2);
      count = size * size;
    } else if (kind == 1) {
      a = d.integer(0, size);
      b = d.integer(0, 2);
      swap = d.integer(0, 2);
      count = size;
    } else {
      len = d.integer(1, size - 1);
      a = d.integer(0, size - len);
      b = d.integer(0, size - len);
#pragma unroll
      for (int s = 0; s < 4; ++s) rev |= d.integer(0, 2) << s;
      // Fisher-Yates from the top on (0, 1, 2, 3), two bits per position
      uint32_t p = 0xE4u;  // 3,2,1,0
#pragma unroll
      for (int i = 3; i >= 1; --i) {
        const int j = d.integer(0, i + 1);
        const uint32_t vi = (p >> (2 * i)) & 3u, vj = (p >> (2 * j)) & 3u;
        p = (p & ~((3u << (2 * i)) | (3u << (2 * j)))) | (vj << (2 * i)) | (vi << (2 * j));
      }
      perm = (int)p;
      count = 4 * (len + 1);
    }
  }

  // entry `step` of the sequence
  __device__ __forceinline__ void entry(int size, int& x, int& y) const {
    if (kind == 0) {
      x = step % size;
      y = step / size;
      if (a) x = size - 1 - x;
      if (b) y = size - 1 - y;
    } else if (kind == 1) {
      x = step;
      y = b ? size - 1 - a : a;
    } else {
      const int q = step / (len + 1), side = (perm >> (2 * q)) & 3;
      int o = step - q * (len + 1);
      if ((rev >> side) & 1) o = len - o;
      x = side == 0 ? a : (side == 1 ? a + len : a + o);
      y = side == 2 ? b : (side == 3 ? b + len : b + o);
      return;
    }
    if (swap) {
      const int t = x;
      x = y;
      y = t;
    }
  }
};

__global__ void __launch_bounds__(kPlayThreads) play_plan_kernel(PlayArgs A) {
  const int64_t e = (int64_t)blockIdx.x * kPlayThreads + threadIdx.x;
  if (e >= A.n) return;
  const ogbx_play_config& c = A.cfg;
  const uint64_t g = (uint64_t)e + (uint64_t)c.env_base;
  PlayDraws d{A.tape ? A.tape + e * A.tape_len : nullptr, A.tape_len, (uint32_t)g, (uint32_t)c.episode,
              (uint32_t)(g >> 32), A.k0, A.k1, 0, false};
  PlayBehavior beh;
  beh.choose(d, c);
  int fresh = 1;
  int held[3] = {0, 0, 0};
  const int T = A.T;
  for (int t = 0; t < T; t += 3) {
    // the decision of stage 0, then the three actions it holds
    const double u = d.uniform();
    const bool random = u < c.p_random;
    int rec = (random ? 1 : 0) | (beh.kind << 1) | (fresh << 3) | (beh.step << 8);
    fresh = 0;
    if (random) {
      held[0] = d.integer(0, c.num_elems);
      held[1] = d.integer(0, c.xy_size);
      held[2] = d.integer(0, c.xy_size);
    } else {
      held[0] = beh.elem;
      beh.entry(c.size, held[1], held[2]);
      beh.step += 1;
      if (beh.step == beh.count) {  // done: replaced in this step
        beh.choose(d, c);
        fresh = 1;
      }
    }
    if (A.out.decisions) A.out.decisions[(int64_t)(t / 3) * A.n + e] = rec;
#pragma unroll
    for (int s = 0; s < 3; ++s)
      if (t + s < T) A.actions[(int64_t)(t + s) * A.n + e] = held[s];
  }
  if (A.out.used) A.out.used[e] = d.used;
  if (d.ran_out) atomicAdd(reinterpret_cast<unsigned long long*>(A.short_count), 1ull);
  if (A.out.terminals && e == 0)
    for (int t = 0; t < T; ++t) A.out.terminals[t] = t == T - 1;
}

__global__ void __launch_bounds__(256) play_semantic_kernel(int32_t ne, int32_t xy, int64_t n, int64_t env_base,
                                                            uint32_t call_lo, uint32_t k0, uint32_t k1,
                                                            int32_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const uint64_t g = (uint64_t)e + (uint64_t)env_base;
  const u32x4 w = philox4x32_10({(uint32_t)g, call_lo, kPlaySemanticSlot, (uint32_t)(g >> 32)}, k0, k1);
  out[3 * e] = (int32_t)bounded_u32(w.x, (uint32_t)ne);
  out[3 * e + 1] = (int32_t)bounded_u32(w.y, (uint32_t)xy);
  out[3 * e + 2] = (int32_t)bounded_u32(w.z, (uint32_t)xy);
}

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_play_api_version(void) { return OGBX_PLAY_API_VERSION; }

ogbx_status ogbx_play_powder_reset(ogbx_powder_t env, const uint8_t* mask, uint8_t* obs, uint64_t seed,
                                   void* stream) {
  OGBX_CHECK(env && obs, OGBX_EINVAL, "ogbx_play_powder_reset: null argument");
  return powder_data_reset(env, mask, obs, seed, stream);
}

ogbx_status ogbx_play_plan(const ogbx_play_config* cfg, int64_t n_envs, int32_t T, int32_t* actions,
                           const ogbx_play_tape* tape, const ogbx_play_outputs* out, uint64_t seed,
                           void* stream) {
  const std::string who = "ogbx_play_plan: ";
  OGBX_CHECK(cfg && actions, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(n_envs > 0 && n_envs <= (1ll << 31), OGBX_EINVAL, who + "n_envs out of range");
  OGBX_CHECK(T > 0, OGBX_EINVAL, who + "T must be > 0");
  OGBX_CHECK(cfg->p_random >= 0.0 && cfg->p_random <= 1.0, OGBX_EINVAL, who + "p_random must be in [0, 1]");
  OGBX_CHECK(cfg->size >= 2 && cfg->size <= 64, OGBX_EINVAL, who + "size must be in 2..64");
  OGBX_CHECK(cfg->num_elems >= 1 && cfg->num_elems <= 64, OGBX_EINVAL, who + "num_elems must be in 1..64");
  OGBX_CHECK(cfg->xy_size >= 1 && cfg->xy_size <= 256, OGBX_EINVAL, who + "xy_size must be in 1..256");
  OGBX_CHECK(cfg->cdf[0] >= 0.0 && cfg->cdf[0] <= cfg->cdf[1] && cfg->cdf[1] <= cfg->cdf[2] && cfg->cdf[2] == 1.0,
             OGBX_EINVAL, who + "cdf must be nondecreasing in [0, 1] and end at 1");
  OGBX_CHECK(cfg->env_base >= 0, OGBX_EINVAL, who + "env_base must be >= 0");
  OGBX_CHECK(!tape || !tape->tape || (tape->tape_len > 0 && tape->short_count), OGBX_EINVAL,
             who + "a tape needs tape_len > 0 and short_count");
  const ogbx_play_outputs o = out ? *out : ogbx_play_outputs{};
  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  bool ok = on_device(actions, dev) && all_on_device(dev, {o.used, o.decisions, o.terminals});
  if (tape && tape->tape) ok = ok && on_device(tape->tape, dev) && on_device(tape->short_count, dev);
  OGBX_CHECK(ok, OGBX_EINVAL, who + "every pointer must be device memory of the current device");

  PlayArgs a{};
  a.cfg = *cfg;
  a.n = n_envs;
  a.T = T;
  a.actions = actions;
  if (tape && tape->tape) {
    a.tape = tape->tape;
    a.tape_len = tape->tape_len;
    a.short_count = tape->short_count;
  }
  a.out = o;
  seed_key(seed, kTagPlayPlan, &a.k0, &a.k1);
  const int64_t blocks = (n_envs + kPlayThreads - 1) / kPlayThreads;
  hipLaunchKernelGGL(play_plan_kernel, dim3((uint32_t)blocks), dim3(kPlayThreads), 0, (hipStream_t)stream, a);
  OGBX_LAUNCHED("play_plan_kernel");
  return OGBX_OK;
}

ogbx_status ogbx_play_sample_semantic(int32_t num_elems, int32_t xy_size, int64_t n_envs, int64_t env_base,
                                      uint64_t seed, uint64_t call_index, int32_t* out, void* stream) {
  const std::string who = "ogbx_play_sample_semantic: ";
  OGBX_CHECK(out, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(n_envs > 0 && n_envs <= (1ll << 31), OGBX_EINVAL, who + "n_envs out of range");
  OGBX_CHECK(num_elems >= 1 && num_elems <= 64 && xy_size >= 1 && xy_size <= 256, OGBX_EINVAL,
             who + "num_elems must be in 1..64 and xy_size in 1..256");
  OGBX_CHECK(env_base >= 0, OGBX_EINVAL, who + "env_base must be >= 0");
  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  OGBX_CHECK(on_device(out, dev), OGBX_EINVAL, who + "out must be device memory of the current device");
  uint32_t k0, k1;
  seed_key(seed, kTagPlayPlan, &k0, &k1);
  hipLaunchKernelGGL(play_semantic_kernel, dim3((uint32_t)((n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     num_elems, xy_size, n_envs, env_base, (uint32_t)call_index, k0, k1, out);
  OGBX_LAUNCHED("play_semantic_kernel");
  return OGBX_OK;
}

}  // extern "C"
