// Phase form of the nearest-x2 upsampler conv (ctrlv_gemm_desc.up = 2, include/ctrlv_hip.h): the ping-pong instantiations, the
// layer predicate and the weight packer.
//
// On the upsampled grid the taps dy = -1, 0, +1 of an output row of parity py read only TWO input rows -- py = 0: row i - 1
// (through w[0]) and row i (through w[1] + w[2]); py = 1: row i (w[0] + w[1]) and row i + 1 (w[2]) -- and the same along x.
// nearest-x2 + 3x3 conv is therefore exactly four 2x2 convs on the low-resolution input, one per output parity (py, px), with
// weights that are sums of 1, 2, 2 and 4 of the original taps: 4 Cin of contraction per output pixel instead of 9 Cin, the
// same bytes.  Zero padding of the high-resolution border is zero padding of the low-resolution input.
#include "gemm_pp_kernel.h"

// 256x320 tile, bias-only epilogue (the consumer's GroupNorm straddles the skip concat: no partials), plain and -- fp16
// element library -- with the split trunk planes.
int ctrlv_gemm_launch_pp_up(const ctrlv_gemm_desc& d, bool persistent, hipStream_t stream) {
  if (pp_split_io(d)) {
#ifdef CTRLV_ELEM_F16
    return launch_one<320, 4, 2, 1, false, 0, false, false, false, false, true, true>(d, persistent, stream);
#else
    ctrlv_set_error("ctrlv_gemm: split trunk planes are served by the fp16 element library only");
    return CTRLV_E_BAD_ARG;
#endif
  }
  return launch_one<320, 4, 2, 1, false, 0, false, false, false, false, false, true>(d, persistent, stream);
}

// A function of the LAYER (Cin, N, H, W, pitches, epilogue operands) and never of the image count: a clip gets the same bits
// alone and in a batch.  The launch itself (ctrlv_gemm, up = 2) also needs its operands inside 32-bit byte offsets
// (ctrlv_gemm_pp_supports) and refuses a batch beyond them.
extern "C" int ctrlv_gemm_up_phase_serves(const ctrlv_gemm_desc* dp) {
  if (!dp || !ctrlv_debug().up_phase) return 0;
  const ctrlv_gemm_desc& d = *dp;
  if (d.mode != 1 || d.taps != 9 || d.stride != 1 || !(d.up == 1 || d.up == 2) || d.pad_br) return 0;
  if (d.H <= 0 || d.Wd <= 0 || d.Ho != 2 * d.H || d.Wo != 2 * d.Wd) return 0;
  if (d.Wd > 256 || (d.Wd & (d.Wd - 1)) != 0) return 0;          // the row remap of the epilogue: Wd divides the 256-row tile
  if (d.Cin <= 0 || d.Cin % 64 != 0 || d.N <= 0 || d.N % 32 != 0) return 0;
  if (d.lda % 8 != 0 || d.ldo % 8 != 0 || d.n_store % 8 != 0) return 0;
  if (d.A2 || d.R1 || d.R2 || d.vmode || d.act || d.geglu || d.out_f32 || d.raw_out || d.gn_partials || d.n_scale2 || d.ksplit) return 0;
  if (d.R1_lo || d.R2_lo) return 0;
  if (d.out_lo && (CTRLV_ELEM_DTYPE != 1 || d.N % 320 != 0)) return 0;   // split planes: launch_epi_split's rule
  return 1;
}

namespace {
__device__ __forceinline__ float up_ld_any(const void* p, int dtype, long i) {
  if (dtype == 0) return ((const float*)p)[i];
  if (dtype == 1) return (float)((const _Float16*)p)[i];
  return bf16_to_f32(((const bf16_t*)p)[i]);
}
// dst[p][n][t * Cin + c], p = 2 py + px, t = 2 a + b = sum over ky in KY(py, a), kx in KY(px, b) of w[n][c][ky][kx] in fp32 (ky outer,
// kx inner, ascending), rounded ONCE to the element type.  KY(0, 0) = {0}, KY(0, 1) = {1, 2}, KY(1, 0) = {0, 1}, KY(1, 1) = {2}.
__global__ void pack_up_phase_kernel(const void* __restrict__ src, int dtype, int N, int Cin, el_t* __restrict__ dst) {
  const long total = 16L * N * Cin;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cin);
    const long r = i / Cin;
    const int t = (int)(r & 3);
    const long pn = r >> 2;
    const int n = (int)(pn % N), p = (int)(pn / N);
    const int py = p >> 1, px = p & 1, a = t >> 1, b = t & 1;
    const int ky0 = py + a == 0 ? 0 : (py + a == 1 ? (py ? 0 : 1) : 2), ky1 = py + a == 1 ? ky0 + 1 : ky0;
    const int kx0 = px + b == 0 ? 0 : (px + b == 1 ? (px ? 0 : 1) : 2), kx1 = px + b == 1 ? kx0 + 1 : kx0;
    const long base = ((long)n * Cin + c) * 9;
    float s = 0.f;
    for (int ky = ky0; ky <= ky1; ++ky)
      for (int kx = kx0; kx <= kx1; ++kx) s += up_ld_any(src, dtype, base + ky * 3 + kx);
    dst[i] = f32_to_el(s);
  }
}
}  // namespace

extern "C" int ctrlv_pack_up_phase_weight(const void* w, int dtype, int N, int Cin, void* dst, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(w && dst, "ctrlv_pack_up_phase_weight: null pointer");
  CTRLV_CHECK_ARG(dtype >= 0 && dtype <= 2, "ctrlv_pack_up_phase_weight: dtype %d (0 fp32, 1 fp16, 2 bf16)", dtype);
  CTRLV_CHECK_SHAPE(N > 0 && Cin > 0, "ctrlv_pack_up_phase_weight: N=%d Cin=%d", N, Cin);
  const long total = 16L * N * Cin;
  const unsigned blocks = (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
  hipLaunchKernelGGL(pack_up_phase_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, dtype, N, Cin, (el_t*)dst);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

CTRLV_CLOCK_READER(pp_up)
