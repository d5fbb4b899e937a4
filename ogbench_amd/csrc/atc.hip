// atc.hip -- ATC batches on gfx950 (include/ogbx_atc.h): anchor / positive
// observation pairs (o_t, o_{t+k}) of one trajectory, frame stacked and
// randomly cropped, in one launch.
//
// Reference (hliuson/ogbench impls/utils/datasets.py):
//   ATCDataset.sample                  401-415
//   ATCDataset.get_valid_atc_idxs      417-436
//   ATCDataset.augment                 438-448
//   ATCDataset.get_stacked_observations 457-464
//
// One workgroup per (sample, side).  Both workgroups of a sample draw the same
// anchor pick and crop offsets (the Philox words are a function of the sample
// and the call), map the pick to a row through the valid(k) table or the
// periodic closed form, take row + k on the positive side, and stage and
// compose their image with visual_tile.h, the code visual_gather_kernel runs.
// What the kernel and ogbx_atc_sample share with the ring's (online_atc.hip)
// is in atc_device.h.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "../../include/ogbx_atc.h"
#include "atc_device.h"
#include "common.h"
#include "gc_device.h"
#include "visual_tile.h"

namespace ogbx {

struct AtcArgs {
  const int64_t* traj_end;
  int64_t num_rows;
  const int64_t* valid;  // valid(k), or NULL: the closed form
  int64_t num_valid;     // size of valid(k) either way
  int64_t period, m;     // closed form: row(p) = (p / m) * period + p % m
  int64_t k;
  const int64_t *idxs, *pick, *crop_from;
  ogbx_atc_outputs out;
  ogbx_atc_column col;
  int32_t frame_stack, padding;
  int32_t draw;
  uint32_t k0, k1, call_lo, call_hi;
  uint32_t lds_bytes;
  int64_t total;
};

__global__ void __launch_bounds__(kVisThreads) atc_sample_kernel(AtcArgs a) {
  extern __shared__ uint4 atc_lds4[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(atc_lds4);
  int side;  // 0 anchor, 1 positive
  const int64_t s = atc_sample_of_block(blockIdx.x, &side);
  if (s >= a.total) return;
  const int t = threadIdx.x;
  const int64_t R = a.num_rows;
  const uint64_t su = (uint64_t)s;
  const uint32_t c0 = (uint32_t)su, c3 = (uint32_t)(su >> 32) ^ a.call_hi;

  int64_t idx, pick = -1;
  bool bad = false;
  if (a.idxs) {
    idx = a.idxs[s];
    bad = idx < 0 || idx >= R;
    idx = clamp_row(idx, R);
    bad = bad || idx + a.k > a.traj_end[idx];
  } else {
    if (a.pick) {
      pick = a.pick[s];
      pick = pick < 0 ? 0 : (pick >= a.num_valid ? a.num_valid - 1 : pick);
    } else {
      const u32x4 w = philox4x32_10({c0, a.call_lo, 0u, c3}, a.k0, a.k1);
      pick = (int64_t)bounded64(w.x, w.y, (uint64_t)a.num_valid);
    }
    if (a.valid) {
      idx = clamp_row(a.valid[pick], R);
    } else {
      const int64_t q = pick / a.m;
      idx = q * a.period + (pick - q * a.m);
    }
  }
  const int64_t r = side ? clamp_row(idx + a.k, R) : idx;
  const int F = a.frame_stack;
  const int64_t start = stack_start(a.traj_end, r, F);

  const int p = a.padding;
  // the crop block and the lane-0 records stay written out in both ATC kernels: a
  // helper moved this kernel's code or the other's (profiles/atc_device_refactor_isa.txt)
  int cy = p, cx = p;  // identity
  if (a.crop_from || a.draw) {
    int64_t oy, ox;
    if (a.crop_from) {
      oy = a.crop_from[2 * s];
      ox = a.crop_from[2 * s + 1];
      // an out-of-range window start moves into range (lax.dynamic_slice)
      oy = oy < 0 ? 0 : (oy > 2 * p ? 2 * p : oy);
      ox = ox < 0 ? 0 : (ox > 2 * p ? 2 * p : ox);
    } else {
      const u32x4 w = philox4x32_10({c0, a.call_lo, (uint32_t)OGBX_VISUAL_CROP_SLOT, c3}, a.k0, a.k1);
      oy = bounded_u32(w.x, (uint32_t)(2 * p + 1));
      ox = bounded_u32(w.y, (uint32_t)(2 * p + 1));
    }
    if (a.col.crop) {
      cy = (int)oy;
      cx = (int)ox;
    }
    if (a.out.crop_from && side == 0 && t == 0) {
      a.out.crop_from[2 * s] = oy;
      a.out.crop_from[2 * s + 1] = ox;
    }
  }
  if (side == 0 && t == 0) {
    if (a.out.idxs) a.out.idxs[s] = idx;
    if (a.out.pick) a.out.pick[s] = pick;
    if (bad && a.out.bad_count) atomicAdd(reinterpret_cast<unsigned long long*>(a.out.bad_count), 1ull);
  }

  const ogbx_atc_column& col = a.col;
  const int orb = col.width * (F * col.px_bytes);  // output row bytes
  uint8_t* dst = static_cast<uint8_t*>(side ? col.positive : col.anchor) + s * ((int64_t)col.height * orb);
  compose_image(lds, a.lds_bytes, VisGeom{col.src, col.height, col.width, col.px_bytes}, r, start, F, cy, cx, p,
                dst);
}

// c + k <= traj_end[c]
struct AtcValid {
  const int64_t* traj_end;
  int64_t k;
  __device__ bool operator()(const int64_t& c) const { return c + k <= traj_end[c]; }
};

template <class It>
static ogbx_status atc_select(It in, int64_t n, const AtcValid& pred, int64_t* out, int64_t* count, hipStream_t s) {
  size_t tmp_bytes = 0;
  OGBX_HIP(hipcub::DeviceSelect::If(nullptr, tmp_bytes, in, out, count, n, pred, s));
  void* tmp = nullptr;
  OGBX_HIP(hipMallocAsync(&tmp, tmp_bytes > 0 ? tmp_bytes : 1, s));
  hipError_t e = hipcub::DeviceSelect::If(tmp, tmp_bytes, in, out, count, n, pred, s);
  hipError_t e2 = hipFreeAsync(tmp, s);
  if (e != hipSuccess) return hip_fail(e, "hipcub::DeviceSelect::If");
  if (e2 != hipSuccess) return hip_fail(e2, "hipFreeAsync");
  return OGBX_OK;
}

}  // namespace ogbx

using namespace ogbx;

extern "C" {

int32_t ogbx_atc_api_version(void) { return OGBX_ATC_API_VERSION; }

ogbx_status ogbx_atc_valid_idxs(const ogbx_gc_buffer* buf, int64_t k, int64_t* out, int64_t* count,
                                void* stream) {
  const std::string who = "ogbx_atc_valid_idxs: ";
  OGBX_CHECK(buf && out && count, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(buf->num_rows > 0 && buf->traj_end, OGBX_EINVAL, who + "empty trajectory buffer");
  OGBX_CHECK(k >= 0, OGBX_EINVAL, who + "k must be >= 0");
  OGBX_CHECK(!buf->valid_idxs || buf->num_valid >= 0, OGBX_EINVAL, who + "negative num_valid");
  const AtcValid pred{buf->traj_end, k};
  hipStream_t s = (hipStream_t)stream;
  if (buf->valid_idxs) {
    if (buf->num_valid == 0) {
      OGBX_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), s));
      return OGBX_OK;
    }
    return atc_select(buf->valid_idxs, buf->num_valid, pred, out, count, s);
  }
  return atc_select(hipcub::CountingInputIterator<int64_t>(0), buf->num_rows, pred, out, count, s);
}

ogbx_status ogbx_atc_sample(const ogbx_gc_buffer* buf, const ogbx_atc_column* col, int64_t total, int64_t k,
                            const int64_t* valid, int64_t num_valid, int32_t frame_stack, int32_t padding,
                            const int64_t* idxs, const int64_t* pick, const int64_t* crop_from,
                            int32_t draw_crop, uint64_t seed, uint64_t call_index,
                            const ogbx_atc_outputs* out, void* stream) {
  const std::string who = "ogbx_atc_sample: ";
  OGBX_CHECK(buf && col, OGBX_EINVAL, who + "null argument");
  OGBX_CHECK(buf->num_rows > 0 && buf->traj_end, OGBX_EINVAL, who + "empty trajectory buffer");
  const AtcCall c{col,       total,     k,    frame_stack, padding, idxs, pick,
                  crop_from, draw_crop, seed, call_index,  out ? *out : ogbx_atc_outputs{}};
  if (ogbx_status st = check_atc_call(who, c)) return st;
  const ogbx_atc_outputs& o = c.out;

  AtcArgs a{};
  if (valid) {
    a.num_valid = num_valid;
  } else if (buf->period > 0) {
    OGBX_CHECK(periodic_ok(*buf), OGBX_EINVAL, who + "inconsistent period fields");
    a.period = buf->period;
    a.m = std::min<int64_t>(buf->period_picks, buf->period_end - k + 1);
    a.num_valid = a.m > 0 ? (buf->num_rows / buf->period) * a.m : 0;
  } else {
    OGBX_CHECK(idxs, OGBX_EINVAL, who + "a valid(k) table is required (the buffer is not periodic)");
  }
  OGBX_CHECK(idxs || a.num_valid > 0, OGBX_EINVAL, who + "valid(k) is empty");

  uint32_t lds = 0;
  int64_t blocks = 0;
  if (ogbx_status st = atc_launch_shape(who, c, &lds, &blocks)) return st;

  int dev = 0;
  OGBX_HIP(hipGetDevice(&dev));
  const bool ok = all_on_device(dev, {buf->traj_end, col->src, col->anchor, col->positive, valid, idxs, pick, crop_from,
                                      o.idxs, o.pick, o.crop_from, o.bad_count});
  OGBX_CHECK(ok, OGBX_EINVAL, who + "every pointer must be device memory of the current device");

  a.traj_end = buf->traj_end;
  a.num_rows = buf->num_rows;
  a.valid = valid;
  fill_atc_args(a, c, lds);
  hipLaunchKernelGGL(atc_sample_kernel, dim3((uint32_t)blocks), dim3(kVisThreads), lds, (hipStream_t)stream, a);
  OGBX_LAUNCHED("atc_sample_kernel");
  return OGBX_OK;
}

}  // extern "C"
