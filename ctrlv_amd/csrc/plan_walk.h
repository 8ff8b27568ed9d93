// What the C++ plan walks share at run time (plan.hip: UNet / ControlNet, vae_plan.hip: VAE encode / decode; the device
// switch also serves clip_plan.hip and weight_loader.hip): the launch gate of a walk that runs twice -- once measuring, once
// live --, the "make the plan's device current for a while" scope and the conv geometry of a GEMM descriptor.  Host code
// only, header only.
#pragma once
#include "common.h"

// (internal to the library: hidden, so the exported symbol set is the C ABI it always was)
namespace ctrlv_walk __attribute__((visibility("hidden"))) {

// Base of a walk context.  The same walk function lays the workspace out (dry: the size query) and runs the forward, so
// every launch goes through run(): nothing is called, and no operand pointer is dereferenced, on the measuring walk.
struct LaunchGate {
  hipStream_t st;
  bool dry;
  template <class Fn>
  int run(Fn&& launch) { return dry ? CTRLV_OK : launch(); }
};

// Makes `device` current if it is not, and the caller's device current again on exit (restore = false: `device` stays).
// status(): for the callers that must fail where the switch failed; the destroy paths ignore it.
struct DeviceScope {
  int device, prev = 0;
  bool back = false;
  hipError_t set_error = hipSuccess;
  explicit DeviceScope(int device_, bool restore = true) : device(device_) {
    const bool known = hipGetDevice(&prev) == hipSuccess;
    if (known && prev == device) return;
    set_error = hipSetDevice(device);
    back = restore && known && set_error == hipSuccess;
  }
  ~DeviceScope() {
    if (back) (void)hipSetDevice(prev);
  }
  int status() const {
    if (set_error == hipSuccess) return CTRLV_OK;
    ctrlv_set_error("hipSetDevice(%d) failed: %s", device, hipGetErrorString(set_error));
    return CTRLV_E_HIP;
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// conv geometry / residual operand of a descriptor made by ctrlv_linear_desc (common.h)
inline void conv2d(ctrlv_gemm_desc& d, int H, int W, int Ho, int Wo, int stride = 1, int up = 0) {
  d.taps = 9; d.mode = 1; d.H = H; d.Wd = W; d.Ho = Ho; d.Wo = Wo; d.stride = stride; d.up = up;
}
inline void conv_t(ctrlv_gemm_desc& d, int F, int S) { d.taps = 3; d.mode = 2; d.F = F; d.S = S; }
inline void resid(ctrlv_gemm_desc& d, const void* R1, int ld) { d.R1 = R1; d.ldr1 = ld; }

}  // namespace ctrlv_walk
