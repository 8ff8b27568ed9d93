// The weight loader of the three plans (weight_loader.h) and ctrlv_pack_weight: PyTorch parameters of any boundary dtype,
// packed ON THE DEVICE into the layouts the kernels consume (include/ctrlv_hip.h: ctrlv_gemm_desc).
#include <math.h>

#include "plan_walk.h"
#include "weight_loader.h"

namespace {

// ------------------------------------------------------------------------------------------------ packing kernels
__device__ __forceinline__ float ld_any(const void* p, int dtype, long i) {
  if (dtype == 0) return ((const float*)p)[i];
  if (dtype == 1) return (float)((const _Float16*)p)[i];
  return bf16_to_f32(((const bf16_t*)p)[i]);
}
// GEGLU row interleave (packing.geglu_interleave): rows [a_0..a_{I-1} | g_0..g_{I-1}] -> alternating 16-row blocks
__device__ __forceinline__ int row_map(int n, int N, int geglu) {
  if (!geglu) return n;
  const int inner = N >> 1, isg = n >= inner, r = isg ? n - inner : n;
  return ((r >> 4) * 2 + isg) * 16 + (r & 15);
}
// dst[(n_off + rowmap(n)) * ld + tap * cp + c_off + c] = src[(n * C + c) * taps + tap]   (dst pre-zeroed)
// covers nn.Linear / 1x1 conv (taps 1), Conv2d 3x3 (taps 9, tap = ky*3+kx), Conv3d (3,1,1) (taps 3), the shared
// conv_in | control_conv_in im2col slots (cp = slot width, c_off = slot offset) and row concatenation (n_off).
__global__ void pack_weight_kernel(const void* __restrict__ src, int dtype, int N, int C, int taps, el_t* __restrict__ dst,
                                   int ld, int cp, int c_off, int n_off, int geglu) {
  const long total = (long)N * C * taps;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int tap = (int)(i % taps);
    const long nc = i / taps;
    const int c = (int)(nc % C), n = (int)(nc / C);
    dst[(long)(n_off + row_map(n, N, geglu)) * ld + tap * cp + c_off + c] = f32_to_el(ld_any(src, dtype, i));
  }
}
// Role-swapped (dgrad) form of a weight: dst[c][(taps - 1 - tap) * Np + n] = src[(n * C + c) * taps + tap]  -- taps
// reversed, output and input channels transposed (autograd.py::gemm_grads); columns n in [N, Np) are zeros.
// A transpose: 32 output rows n x 64 consecutive (c, tap) source elements per workgroup go through LDS, so that reads are
// contiguous along a source row and writes are 32 consecutive n (64 B) per (c, tap).   grid (ceil(C*taps/64), ceil(Np/32))
__global__ __launch_bounds__(256) void pack_weight_swapped_kernel(const void* __restrict__ src, int dtype, int N, int C,
                                                                  int taps, int Np, el_t* __restrict__ dst, int ld) {
  __shared__ float tile[32][65];
  const int k0 = blockIdx.x * 64, n0 = blockIdx.y * 32, ktot = C * taps;
  for (int i = threadIdx.x; i < 32 * 64; i += 256) {
    const int r = i >> 6, kk = i & 63, n = n0 + r, k = k0 + kk;
    tile[r][kk] = (n < N && k < ktot) ? ld_any(src, dtype, (long)n * ktot + k) : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 32; i += 256) {
    const int kk = i >> 5, r = i & 31, k = k0 + kk, n = n0 + r;
    if (k >= ktot || n >= Np) continue;
    const int c = k / taps, tap = k - c * taps;
    dst[(long)c * ld + (long)(taps - 1 - tap) * Np + n] = f32_to_el(tile[r][kk]);
  }
}
// Forward form with coalesced writes: dst[rowmap(n)][tap * C + c] = src[(n * C + c) * taps + tap]   grid (ceil(taps*C/256), N)
__global__ void pack_weight_rows_kernel(const void* __restrict__ src, int dtype, int N, int C, int taps,
                                        el_t* __restrict__ dst, int ld, int geglu) {
  const int n = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= taps * C) return;
  const int tap = k / C, c = k - tap * C;
  dst[(long)row_map(n, N, geglu) * ld + k] = f32_to_el(ld_any(src, dtype, ((long)n * C + c) * taps + tap));
}
// dst[n_off + rowmap(n)] (+)= src[n] in fp32.  N may exceed 2^31 only without the GEGLU interleave (whole tables: CLIP's
// position_embedding, the VAE's quant_conv.weight).
__global__ void pack_vector_kernel(const void* __restrict__ src, int dtype, long N, float* __restrict__ dst, int n_off,
                                   int geglu, int accumulate) {
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long)gridDim.x * blockDim.x) {
    const float v = ld_any(src, dtype, n);
    float* d = dst + n_off + (geglu ? (long)row_map((int)n, (int)N, geglu) : n);
    *d = accumulate ? *d + v : v;
  }
}

inline unsigned blocks_for(long total) { return (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535); }
inline size_t elem_bytes(int dtype) { return dtype == 0 ? 4 : 2; }

}  // namespace

namespace ctrlv_load {

void WeightLoader::add(const ctrlv_tensor_desc* tensors, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (tensors[i].name) map[tensors[i].name] = &tensors[i];
}

int WeightLoader::find(const std::string& name, long numel, const ctrlv_tensor_desc** out) {
  auto it = map.find(name);
  if (it == map.end()) { ctrlv_set_error("%s: missing tensor '%s'", who, name.c_str()); return CTRLV_E_BAD_ARG; }
  const ctrlv_tensor_desc* t = it->second;
  if (numel >= 0 && t->numel != numel) {
    ctrlv_set_error("%s: '%s' has %ld elements, expected %ld", who, name.c_str(), (long)t->numel, numel);
    return CTRLV_E_BAD_SHAPE;
  }
  CTRLV_CHECK_DTYPE(t->dtype >= 0 && t->dtype <= 2 && t->data, "%s: '%s': dtype code %d / null data", who, name.c_str(), t->dtype);
  *out = t;
  return CTRLV_OK;
}

int WeightLoader::dev_ptr(const ctrlv_tensor_desc* t, const void** out) {
  if (t->on_device) { *out = t->data; return CTRLV_OK; }
  const size_t bytes = (size_t)t->numel * elem_bytes(t->dtype);
  void* d = nullptr;
  CTRLV_HIP_TRY(hipMalloc(&d, bytes));
  staged.push_back(d);
  CTRLV_HIP_TRY(hipMemcpy(d, t->data, bytes, hipMemcpyHostToDevice));
  *out = d;
  return CTRLV_OK;
}

int WeightLoader::host_f32(const std::string& name, long numel, std::vector<float>& out) {
  const ctrlv_tensor_desc* t;
  CTRLV_TRY(find(name, numel, &t));
  const size_t bytes = (size_t)t->numel * elem_bytes(t->dtype);
  std::vector<char> raw(bytes);
  if (t->on_device) CTRLV_HIP_TRY(hipMemcpy(raw.data(), t->data, bytes, hipMemcpyDeviceToHost));
  else memcpy(raw.data(), t->data, bytes);
  out.resize((size_t)t->numel);
  for (size_t i = 0; i < out.size(); ++i) {
    if (t->dtype == 0) { memcpy(&out[i], raw.data() + 4 * i, 4); continue; }
    uint16_t h;
    memcpy(&h, raw.data() + 2 * i, 2);
    if (t->dtype == 1) out[i] = (float)__builtin_bit_cast(_Float16, h);
    else { const uint32_t u = (uint32_t)h << 16; memcpy(&out[i], &u, 4); }
  }
  return CTRLV_OK;
}

int WeightLoader::mix_alpha(const std::string& name, double* alpha) {
  std::vector<float> v;
  CTRLV_TRY(host_f32(name, 1, v));
  *alpha = 1.0 / (1.0 + exp(-(double)v[0]));
  return CTRLV_OK;
}

int WeightLoader::alloc(size_t bytes, void** out, bool zero) {
  void* d = nullptr;
  CTRLV_HIP_TRY(hipMalloc(&d, bytes ? bytes : 256));
  owned->push_back(d);
  if (zero) CTRLV_HIP_TRY(hipMemsetAsync(d, 0, bytes ? bytes : 256, st));
  *out = d;
  return CTRLV_OK;
}

int WeightLoader::upload(const std::vector<float>& v, float** dst) {
  CTRLV_TRY(alloc(v.size() * 4, (void**)dst, false));
  CTRLV_HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * 4, hipMemcpyHostToDevice));
  return CTRLV_OK;
}

int WeightLoader::new_linear(PackedLinear& l, int rows, int k_total, bool bias) {
  l.n = pad_to(rows, 32);
  l.k = k_total;
  CTRLV_TRY(alloc((size_t)l.n * l.k * 2, (void**)&l.w, true));
  l.b = nullptr;
  if (bias) CTRLV_TRY(alloc((size_t)l.n * 4, (void**)&l.b, true));
  return CTRLV_OK;
}

int WeightLoader::pack_w(const std::string& name, int N, int C, int taps, PackedLinear& dst, int cp, int c_off, int n_off,
                         int geglu) {
  const long total = (long)N * C * taps;
  const ctrlv_tensor_desc* t;
  CTRLV_TRY(find(name, total, &t));
  const void* src;
  CTRLV_TRY(dev_ptr(t, &src));
  hipLaunchKernelGGL(pack_weight_kernel, dim3(blocks_for(total)), dim3(256), 0, st, src, t->dtype, N, C, taps, dst.w, dst.k,
                     cp, c_off, n_off, geglu);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int WeightLoader::pack_v(const std::string& name, long N, float* dst, int n_off, int geglu, int accumulate) {
  const ctrlv_tensor_desc* t;
  CTRLV_TRY(find(name, N, &t));
  const void* src;
  CTRLV_TRY(dev_ptr(t, &src));
  hipLaunchKernelGGL(pack_vector_kernel, dim3(blocks_for(N)), dim3(256), 0, st, src, t->dtype, N, dst, n_off, geglu,
                     accumulate);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

int WeightLoader::vec(const std::string& name, long n, float** dst, long n_pad) {
  CTRLV_TRY(alloc((size_t)(n_pad > n ? n_pad : n) * 4, (void**)dst, n_pad > n));
  return pack_v(name, n, *dst, 0, 0, 0);
}

int WeightLoader::linear(const std::string& mod, int N, int K, PackedLinear& l, bool bias, int geglu) {
  CTRLV_TRY(new_linear(l, N, pad_to(K, 64), bias));
  CTRLV_TRY(pack_w(mod + ".weight", N, K, 1, l, 0, 0, 0, geglu));
  if (bias) CTRLV_TRY(pack_v(mod + ".bias", N, l.b, 0, geglu, 0));
  return CTRLV_OK;
}

int WeightLoader::conv3x3(const std::string& mod, int N, int C, PackedLinear& l) {
  CTRLV_TRY(new_linear(l, N, 9 * C, true));
  CTRLV_TRY(pack_w(mod + ".weight", N, C, 9, l, C, 0, 0, 0));
  return pack_v(mod + ".bias", N, l.b, 0, 0, 0);
}

int WeightLoader::conv_t(const std::string& mod, int N, int C, PackedLinear& l) {
  CTRLV_TRY(new_linear(l, N, 3 * C, true));
  CTRLV_TRY(pack_w(mod + ".weight", N, C, 3, l, C, 0, 0, 0));
  return pack_v(mod + ".bias", N, l.b, 0, 0, 0);
}

int WeightLoader::conv_in(const std::string& mod, int N, int C, int c_total, PackedLinear& l, int* cp, int* kp) {
  *cp = pad_to(c_total, 8);
  *kp = pad_to(9 * *cp, 64);
  CTRLV_TRY(new_linear(l, N, *kp, true));
  CTRLV_TRY(pack_w(mod + ".weight", N, C, 9, l, *cp, 0, 0, 0));
  return pack_v(mod + ".bias", N, l.b, 0, 0, 0);
}

int WeightLoader::norm(const std::string& mod, int C, NormParams& nm) {
  CTRLV_TRY(vec(mod + ".weight", C, &nm.g));
  return vec(mod + ".bias", C, &nm.b);
}

int run_load(WeightLoader& L, int device, bool restore_device, const std::function<int()>& body) {
  ctrlv_walk::DeviceScope on(device, restore_device);
  CTRLV_TRY(on.status());
  int rc = body();
  const hipError_t e = hipDeviceSynchronize();
  for (void* d : L.staged) (void)hipFree(d);
  L.staged.clear();
  if (rc == CTRLV_OK && e != hipSuccess) {
    ctrlv_set_error("%s: %s", L.who, hipGetErrorString(e));
    rc = CTRLV_E_HIP;
  }
  return rc;
}

}  // namespace ctrlv_load

extern "C" int ctrlv_pack_weight(const void* src, int src_dtype, int N, int C, int taps, int form, int geglu, void* dst,
                                 int ld_dst, ctrlv_stream_t stream) {
  CTRLV_CHECK_ARG(src && dst, "pack_weight: null pointer");
  CTRLV_CHECK_ARG(src_dtype >= 0 && src_dtype <= 2 && (form == 0 || form == 1), "pack_weight: bad dtype / form");
  CTRLV_CHECK_SHAPE(N > 0 && C > 0 && taps > 0 && N <= 65535 && C <= 65535, "pack_weight: bad shape");
  if (form == 0) {
    CTRLV_CHECK_SHAPE(ld_dst >= taps * C && (!geglu || N % 32 == 0), "pack_weight: ld_dst < taps * C (or odd GEGLU rows)");
    hipLaunchKernelGGL(pack_weight_rows_kernel, dim3((taps * C + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, src,
                       src_dtype, N, C, taps, (el_t*)dst, ld_dst, geglu);
  } else {
    CTRLV_CHECK_SHAPE(ld_dst % taps == 0 && ld_dst / taps >= N && !geglu, "pack_weight: ld_dst must be taps * Np, Np >= N");
    const int Np = ld_dst / taps;
    hipLaunchKernelGGL(pack_weight_swapped_kernel, dim3((taps * C + 63) / 64, (Np + 31) / 32), dim3(256), 0,
                       (hipStream_t)stream, src, src_dtype, N, C, taps, Np, (el_t*)dst, ld_dst);
  }
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}
