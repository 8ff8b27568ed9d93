// Between the box predictor and Box2Video (gfx950): what the reference's tools/eval_overall.py:96-112,154 does on the host in
// numpy between its two pipeline calls, as two memory-bound one-pass kernels.
//   ctrlv_box_frames_post   decoded frames -> the [0, 1] frames of tensor2vid(..., "pt"), the [-1, 1] condition of stage 2 and
//                           the cleaned uint8 box frames (dark pixels and box-less interior frames zeroed)
//   ctrlv_mask_counts       the three pixel counts binary_mask_iou divides (src/ctrlv/metrics/FandJ.py:11-23)
// Where torch / numpy round after every operation the roundings are kept (round_to_el, __fmul_rn / __fadd_rn: no contraction into
// an fma).  Sixteen pixels per thread through 16-byte loads and stores where a plane's H W is a multiple of 16 and the pointers
// are 16-byte aligned, one pixel per thread otherwise.  Wave reductions first, one atomic per workgroup and value.
#include "common.h"

namespace {

constexpr int kThreads = 256;

// fp32 -> element as its OWN rounding (as csrc/pipeline_io.hip: the empty asm keeps the fp32 operation in front of it from being
// folded into a mixed-precision instruction that rounds once)
__device__ __forceinline__ el_t round_to_el(float v) {
  asm volatile("" : "+v"(v));
  return f32_to_el(v);
}

struct Pixel {          // one channel value of one pixel through the three recipes
  el_t pt, cond;
  float v;              // (float) y * 255
};

__device__ __forceinline__ Pixel recipe(el_t x) {
  Pixel p;
  // y = (x / 2 + 0.5).clamp(0, 1): torch divides by a host scalar as a multiplication by its reciprocal, in fp32, and rounds
  const float half = el_to_f32(round_to_el(__fmul_rn(el_to_f32(x), 0.5f)));
  const el_t s = round_to_el(__fadd_rn(half, 0.5f));
  const float sf = el_to_f32(s);
  p.pt = sf < 0.0f ? f32_to_el(0.0f) : (sf > 1.0f ? f32_to_el(1.0f) : s);          // (a NaN stays, as torch.clamp leaves it)
  const float y = el_to_f32(p.pt);
  // 2 * (y - 0.5)
  p.cond = round_to_el(__fmul_rn(2.0f, el_to_f32(round_to_el(__fsub_rn(y, 0.5f)))));
  p.v = __fmul_rn(y, 255.0f);
  return p;
}

// minimum over the workgroup of a non-negative float, one atomic on its bits (which order as the values do)
__device__ __forceinline__ void block_min_to(float m, unsigned* dst) {
  __shared__ float part[kThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) m = fminf(m, part[w]);
    atomicMin(dst, __float_as_uint(m));
  }
}

// One workgroup works inside ONE frame: blockIdx.x = frame * groups + group.  VEC = 16: a thread owns 16 consecutive pixels of
// the frame's three channel planes (HW % 16 == 0, aligned pointers); VEC = 1: one pixel.
template <int VEC>
__global__ __launch_bounds__(kThreads) void box_frames_post_kernel(const el_t* __restrict__ frames, long HW, int groups,
                                                                    float threshold, el_t* __restrict__ out_pt,
                                                                    el_t* __restrict__ out_cond, uint8_t* __restrict__ out_u8,
                                                                    unsigned* __restrict__ frame_min) {
  const long frame = blockIdx.x / groups;
  const long p0 = ((long)(blockIdx.x % groups) * kThreads + threadIdx.x) * VEC;
  const bool live = p0 < HW;
  float lo = __uint_as_float(0x7f7f7f7fu);              // (the fill of frame_min: above every sum, at most 765)
  if (live) {
    const long at = frame * 3 * HW + p0;
    __attribute__((aligned(16))) el_t x[3][VEC];
    if constexpr (VEC == 16) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint4* src = (const uint4*)(frames + at + c * HW);
        *(uint4*)&x[c][0] = src[0];
        *(uint4*)&x[c][8] = src[1];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c][0] = frames[at + c * HW];
    }
    __attribute__((aligned(16))) el_t pt[3][VEC], cd[3][VEC];
    __attribute__((aligned(16))) uint8_t u8[3][VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const Pixel q = recipe(x[c][k]);
        pt[c][k] = q.pt;
        cd[c][k] = q.cond;
        v[c] = q.v;
      }
      const float sum = __fadd_rn(__fadd_rn(v[0], v[1]), v[2]);
      lo = fminf(lo, sum);
      const bool dark = sum < threshold;
#pragma unroll
      for (int c = 0; c < 3; ++c) u8[c][k] = dark ? (uint8_t)0 : (uint8_t)(int)v[c];      // v in [0, 255]: truncation
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long o = at + c * HW;
      if constexpr (VEC == 16) {
        if (out_pt) {
          ((uint4*)(out_pt + o))[0] = *(const uint4*)&pt[c][0];
          ((uint4*)(out_pt + o))[1] = *(const uint4*)&pt[c][8];
        }
        if (out_cond) {
          ((uint4*)(out_cond + o))[0] = *(const uint4*)&cd[c][0];
          ((uint4*)(out_cond + o))[1] = *(const uint4*)&cd[c][8];
        }
        if (out_u8) *(uint4*)(out_u8 + o) = *(const uint4*)&u8[c][0];
      } else {
        if (out_pt) out_pt[o] = pt[c][0];
        if (out_cond) out_cond[o] = cd[c][0];
        if (out_u8) out_u8[o] = u8[c][0];
      }
    }
  }
  if (out_u8) block_min_to(lo, frame_min + frame);
}

// The frame rule, after the pass above has left every frame's minimum channel sum: an interior frame whose minimum is above
// the threshold holds no dark pixel, so no box was drawn over black -- the reference zeroes it.  blockIdx.x = (clip, interior
// frame, group); a frame that stays costs one 4-byte read per workgroup.
__global__ __launch_bounds__(kThreads) void box_frames_blank_kernel(const unsigned* __restrict__ frame_min, int F, int groups,
                                                                     long bytes, float threshold, int vec,
                                                                     uint8_t* __restrict__ out_u8) {
  const long fi = blockIdx.x / groups;                   // over (clip, f - 1), f in [1, F - 2]
  const long frame = fi / (F - 2) * F + fi % (F - 2) + 1;
  if (!(__uint_as_float(frame_min[frame]) > threshold)) return;
  const long t = (long)(blockIdx.x % groups) * kThreads + threadIdx.x;
  uint8_t* dst = out_u8 + frame * bytes;
  if (vec) {
    if (t * 16 < bytes) *(uint4*)(dst + t * 16) = make_uint4(0u, 0u, 0u, 0u);
  } else if (t < bytes) {
    dst[t] = 0;
  }
}

// bytes of a 32-bit word that are nonzero, as their top bits
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u; }

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One workgroup works inside one frame (blockIdx.x = frame * groups + group); VEC as above.  counts [clip][2][3].
template <int VEC>
__global__ __launch_bounds__(kThreads) void mask_counts_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pred,
                                                                long HW, int groups, int F,
                                                                unsigned long long* __restrict__ counts) {
  const long frame = blockIdx.x / groups;
  const long p0 = ((long)(blockIdx.x % groups) * kThreads + threadIdx.x) * VEC;
  unsigned n[3] = {0u, 0u, 0u};                          // gt, pred, both
  if (p0 < HW) {
    const long at = frame * 3 * HW + p0;
    if constexpr (VEC == 16) {
      uint4 a = *(const uint4*)(gt + at), b = *(const uint4*)(pred + at);
#pragma unroll
      for (int c = 1; c < 3; ++c) {
        const uint4 a2 = *(const uint4*)(gt + at + c * HW), b2 = *(const uint4*)(pred + at + c * HW);
        a.x |= a2.x; a.y |= a2.y; a.z |= a2.z; a.w |= a2.w;
        b.x |= b2.x; b.y |= b2.y; b.z |= b2.z; b.w |= b2.w;
      }
      const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t ma = nonzero_bytes(wa[k]), mb = nonzero_bytes(wb[k]);
        n[0] += __popc(ma);
        n[1] += __popc(mb);
        n[2] += __popc(ma & mb);
      }
    } else {
      const bool ma = (gt[at] | gt[at + HW] | gt[at + 2 * HW]) != 0, mb = (pred[at] | pred[at + HW] | pred[at + 2 * HW]) != 0;
      n[0] = ma;
      n[1] = mb;
      n[2] = ma && mb;
    }
  }
  __shared__ unsigned part[kThreads / 64][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned s = wave_sum(n[k]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += part[w][threadIdx.x];
    const long clip = frame / F;
    const int f = (int)(frame % F);
    if (s) {
      atomicAdd(&counts[clip * 6 + threadIdx.x], s);
      if (f == 0 || f == F - 1) atomicAdd(&counts[clip * 6 + 3 + threadIdx.x], s);
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_geometry(const char* who, int n, int F, int H, int W, int vec, long* HW, int* groups) {
  CTRLV_CHECK_SHAPE(n > 0 && F > 0 && H > 0 && W > 0, "%s: n, F, H, W must be positive (got %d, %d, %d, %d)", who, n, F, H, W);
  *HW = (long)H * W;
  const long g = (*HW / vec + kThreads - 1) / kThreads;
  CTRLV_CHECK_SHAPE(g * n * F <= 0x7fffffffL, "%s: %d x %d frames of %d x %d pixels need more than 2^31 - 1 workgroups", who, n, F,
                    H, W);
  *groups = (int)g;
  return CTRLV_OK;
}

}  // namespace

extern "C" size_t ctrlv_box_frames_post_ws_bytes(int n, int F) {
  if (n <= 0 || F <= 0) {
    ctrlv_set_error("box_frames_post_ws_bytes: n=%d, F=%d must be positive", n, F);
    return 0;
  }
  return (size_t)n * F * sizeof(unsigned);
}

extern "C" int ctrlv_box_frames_post(const void* frames, int n, int F, int H, int W, float threshold, void* out_pt, void* out_cond,
                                     void* out_u8, void* ws, size_t ws_bytes, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(frames != nullptr, "box_frames_post: frames is null");
  CTRLV_CHECK_ARG(out_pt || out_cond || out_u8, "box_frames_post: all three outputs are null");
  CTRLV_CHECK_ARG(threshold == threshold, "box_frames_post: threshold is NaN");
  const long plane = (long)H * W;
  const bool vec = H > 0 && W > 0 && plane % 16 == 0 && aligned16(frames) && aligned16(out_pt) && aligned16(out_cond) &&
                   aligned16(out_u8);
  long HW = 0;
  int groups = 0;
  CTRLV_TRY(check_geometry("box_frames_post", n, F, H, W, vec ? 16 : 1, &HW, &groups));
  const hipStream_t s = (hipStream_t)stream;
  unsigned* frame_min = (unsigned*)ws;
  if (out_u8) {
    const size_t need = ctrlv_box_frames_post_ws_bytes(n, F);
    CTRLV_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 3) == 0, "box_frames_post: ws must be non-null and 4-byte aligned when out_u8 "
                    "is asked for");
    if (ws_bytes < need) {
      ctrlv_set_error("box_frames_post: ws_bytes=%zu is smaller than the %zu bytes of ctrlv_box_frames_post_ws_bytes", ws_bytes, need);
      return CTRLV_E_WORKSPACE;
    }
    CTRLV_HIP_TRY(hipMemsetAsync(frame_min, 0x7f, need, s));      // 0x7f7f7f7f = 3.4e38: above every sum
  }
  const dim3 grid((unsigned)((long)groups * n * F));
  if (vec)
    hipLaunchKernelGGL(box_frames_post_kernel<16>, grid, dim3(kThreads), 0, s, (const el_t*)frames, HW, groups, threshold,
                       (el_t*)out_pt, (el_t*)out_cond, (uint8_t*)out_u8, frame_min);
  else
    hipLaunchKernelGGL(box_frames_post_kernel<1>, grid, dim3(kThreads), 0, s, (const el_t*)frames, HW, groups, threshold,
                       (el_t*)out_pt, (el_t*)out_cond, (uint8_t*)out_u8, frame_min);
  CTRLV_LAUNCH_CHECK();
  if (out_u8 && F > 2) {
    const long bytes = 3 * HW;
    const int bvec = bytes % 16 == 0 && aligned16(out_u8) ? 1 : 0;
    const long bg = ((bvec ? bytes / 16 : bytes) + kThreads - 1) / kThreads;
    CTRLV_CHECK_SHAPE(bg * n * (F - 2) <= 0x7fffffffL, "box_frames_post: %d x %d frames of %d x %d pixels need more than 2^31 - 1 "
                      "workgroups", n, F, H, W);
    hipLaunchKernelGGL(box_frames_blank_kernel, dim3((unsigned)(bg * n * (F - 2))), dim3(kThreads), 0, s, frame_min, F, (int)bg,
                       bytes, threshold, bvec, (uint8_t*)out_u8);
    CTRLV_LAUNCH_CHECK();
  }
  return CTRLV_OK;
}

extern "C" int ctrlv_mask_counts(const void* gt_u8, const void* pred_u8, int n, int F, int H, int W, unsigned long long* counts,
                                 ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(gt_u8 && pred_u8 && counts, "mask_counts: null pointer");
  CTRLV_CHECK_ARG(((uintptr_t)counts & 7) == 0, "mask_counts: counts must be 8-byte aligned");
  const bool vec = H > 0 && W > 0 && ((long)H * W) % 16 == 0 && aligned16(gt_u8) && aligned16(pred_u8);
  long HW = 0;
  int groups = 0;
  CTRLV_TRY(check_geometry("mask_counts", n, F, H, W, vec ? 16 : 1, &HW, &groups));
  const hipStream_t s = (hipStream_t)stream;
  CTRLV_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n * 6 * sizeof(unsigned long long), s));
  const dim3 grid((unsigned)((long)groups * n * F));
  if (vec)
    hipLaunchKernelGGL(mask_counts_kernel<16>, grid, dim3(kThreads), 0, s, (const uint8_t*)gt_u8, (const uint8_t*)pred_u8, HW,
                       groups, F, counts);
  else
    hipLaunchKernelGGL(mask_counts_kernel<1>, grid, dim3(kThreads), 0, s, (const uint8_t*)gt_u8, (const uint8_t*)pred_u8, HW, groups,
                       F, counts);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
