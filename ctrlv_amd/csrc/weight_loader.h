// Load-time machinery shared by the UNet / ControlNet, VAE and CLIP plans (plan.hip, vae_plan.hip, clip_plan.hip): the
// name -> tensor lookup with its errors, staging of host tensors, library-owned allocations and the on-device packing of
// PyTorch parameters into the layouts the kernels consume.  Host-side declarations only: the kernels live in weight_loader.hip
// (the library is built without relocatable device code).
#pragma once
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

// (internal to the library: hidden, so the exported symbol set is the C ABI it always was)
namespace ctrlv_load __attribute__((visibility("hidden"))) {

// packed GEMM weight: elements [n][k] (n % 32 == 0; k % 64 == 0 for taps == 1) + fp32 bias [n] (or null)
struct PackedLinear {
  el_t* w = nullptr;
  float* b = nullptr;
  int n = 0, k = 0;      // padded rows, total K (taps * channel slot, padded)
};
struct NormParams { float* g = nullptr; float* b = nullptr; };

struct WeightLoader {
  const char* who;                  // prefix of every error message: the entry point's name
  std::vector<void*>* owned;        // the plan's list of device allocations; alloc() appends to it
  std::unordered_map<std::string, const ctrlv_tensor_desc*> map;
  std::vector<void*> staged;        // temporary device copies of host tensors (run_load frees them)
  hipStream_t st = nullptr;

  WeightLoader(const char* who_, std::vector<void*>* owned_) : who(who_), owned(owned_) {}
  void add(const ctrlv_tensor_desc* tensors, size_t n);      // (nameless descriptors are skipped)

  // descriptor of `name` with exactly `numel` elements (numel < 0: any count), a dtype code in 0..2 and non-null data
  int find(const std::string& name, long numel, const ctrlv_tensor_desc** out);
  int dev_ptr(const ctrlv_tensor_desc* t, const void** out);                    // device address; host tensors are staged
  int host_f32(const std::string& name, long numel, std::vector<float>& out);   // fp32 host copy, from host or device memory
  int mix_alpha(const std::string& name, double* alpha);                        // sigmoid of a scalar (AlphaBlender.mix_factor)
  int alloc(size_t bytes, void** out, bool zero);                               // library-owned, at least 256 bytes
  int upload(const std::vector<float>& v, float** dst);
  // storage of a packed weight: rows padded to 32, k_total as given, both zeroed
  int new_linear(PackedLinear& l, int rows, int k_total, bool bias);
  // one weight tensor [N][C][taps] -> rows [n_off, n_off + N) of dst, element (n, c, tap) at column tap * cp + c_off + c
  int pack_w(const std::string& name, int N, int C, int taps, PackedLinear& dst, int cp, int c_off, int n_off, int geglu);
  // one vector [N] -> dst[n_off + n] in fp32 (added to what is there if `accumulate`)
  int pack_v(const std::string& name, long N, float* dst, int n_off, int geglu, int accumulate);
  // a fresh fp32 copy of a tensor of n elements in max(n, n_pad) floats (the padding zeroed)
  int vec(const std::string& name, long n, float** dst, long n_pad = 0);

  int linear(const std::string& mod, int N, int K, PackedLinear& l, bool bias = true, int geglu = 0);   // [N][K] -> [N32][K64]
  int conv3x3(const std::string& mod, int N, int C, PackedLinear& l);           // k = (ky * 3 + kx) * C + c
  int conv_t(const std::string& mod, int N, int C, PackedLinear& l);            // k = t * C + c
  // first slot of an im2col input conv whose rows hold c_total channels: *cp = slot width (x8), *kp = 9 slots padded to 64
  int conv_in(const std::string& mod, int N, int C, int c_total, PackedLinear& l, int* cp, int* kp);
  int norm(const std::string& mod, int C, NormParams& nm);
};

// The common shape of the *_load_weights entry points: make `device` current, run `body`, wait for the device, free the
// staged copies and (restore_device) make the caller's device current again.  Returns the body's status, or CTRLV_E_HIP
// where the device reported an error; on any failure the caller unloads its plan.
int run_load(WeightLoader& L, int device, bool restore_device, const std::function<int()>& body);

}  // namespace ctrlv_load
