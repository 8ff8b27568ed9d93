// Box and trajectory frames drawn from coordinates (gfx950): what the reference draws on the host with OpenCV
// (src/ctrlv/utils/plotting.py:33-124) and takes through Resize -> ToTensor -> Normalize (datasets/kitti_abstract.py:92-96).
//   ctrlv_render_box_frames     the two device tables -> (n_frames, 3, Hs, Ws) uint8, planar
//   ctrlv_box_frames_cond       render, ctrlv_resize_frames_u8 (BILINEAR), (v / 255 - 0.5) / 0.5 -> the ControlNet's condition
//   ctrlv_box_class_color, ctrlv_box_track_color, ctrlv_box_project_corners    host-only helpers for filling the tables
// The picture is the integer geometry include/ctrlv_hip.h states (tests/box_render_ref.py restates it in numpy); it is NOT claimed
// to be OpenCV's raster.  Everything is 32-bit integer arithmetic on the VALU: with coordinates clamped to +-8191 and pixels below
// 4096 + a tile, every dot and cross product stays below 2^29, and the one comparison that needs more -- 4 (d x e)^2 <= R4 L -- is
// false whenever |d x e| >= 2^15 (R4 L < 2^32 / 2), so it is decided in 32 bits too.
//
// One workgroup (4 waves) per 128 x 32 tile of a frame.  Per round of 256 objects: every thread clamps one object and tests its
// extent against the tile, a wave ballot and a prefix over the four waves give each survivor its slot, and the clamped records go
// into LDS in table order (painter's order is part of the contract).  Then every lane walks that list for its 4 x 4 pixels (four
// consecutive x in four consecutive rows; a wave covers 128 x 8), keeping the three layers in registers across the rounds.  A
// frame's objects that miss the tile cost one extent test per workgroup, not 18 capsule tests per pixel.
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 128, kTileH = 32;      // 32 lanes x 4 pixels; 8 row groups x 4 rows
constexpr int kMaxCount = 1024;               // objects of one frame
constexpr int kClamp = 8191;
constexpr int kMaxSide = 4096;

struct Rec {                 // a surviving object in LDS: coordinates clamped, the box ordered, colours packed r | g << 8 | b << 16
  int xa, xb, ya, yb;
  uint32_t fill, line, flags, pad;
  short cx[8], cy[8];
};
static_assert(sizeof(Rec) == 64, "Rec");
static_assert(sizeof(ctrlv_box_object) == 64 && sizeof(ctrlv_box_frame) == 16, "the records of include/ctrlv_hip.h");

__device__ __forceinline__ int clampc(int v) { return v < -kClamp ? -kClamp : (v > kClamp ? kClamp : v); }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// The four pixels (qx .. qx + 3, qy) against capsule(P0, P1, R4): bit i = pixel i is covered.  t and the cross product move by
// dx and -dy per pixel.
__device__ __forceinline__ unsigned capsule4(int p0x, int p0y, int p1x, int p1y, unsigned R4, int qx, int qy) {
  const int dx = p1x - p0x, dy = p1y - p0y, L = dx * dx + dy * dy;
  int ex = qx - p0x;
  const int ey = qy - p0y;
  int t = dx * ex + dy * ey, c = dx * ey - dy * ex;
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bool cov;
    if (L == 0 || t <= 0) {
      cov = (unsigned)(4 * (ex * ex + ey * ey)) <= R4;
    } else if (t >= L) {
      const int fx = ex - dx, fy = ey - dy;
      cov = (unsigned)(4 * (fx * fx + fy * fy)) <= R4;
    } else {
      const unsigned a = (unsigned)(c < 0 ? -c : c);
      cov = a < 32768u && 4u * a * a <= R4 * (unsigned)L;
    }
    m |= (cov ? 1u : 0u) << i;
    ++ex; t += dx; c -= dy;
  }
  return m;
}

// capsule(P0, P1, R4) onto the lane's 4 x 4 pixels of one layer.  The extent test only skips work: a covered pixel lies within 1
// of the segment.
__device__ __forceinline__ void draw_capsule(uint32_t (&lyr)[4][4], uint32_t color, int p0x, int p0y, int p1x, int p1y, unsigned R4,
                                             int qx, int qy) {
  if (qx + 3 < imin(p0x, p1x) - 1 || qx > imax(p0x, p1x) + 1 || qy + 3 < imin(p0y, p1y) - 1 || qy > imax(p0y, p1y) + 1) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned m = capsule4(p0x, p0y, p1x, p1y, R4, qx, qy + k);
#pragma unroll
    for (int i = 0; i < 4; ++i) lyr[k][i] = (m >> i) & 1u ? color : lyr[k][i];
  }
}

// the closed disc |q - C|^2 <= r2
__device__ __forceinline__ void draw_disc(uint32_t (&lyr)[4][4], uint32_t color, int cx, int cy, int r2, int qx, int qy) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ey = qy + k - cy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ex = qx + i - cx;
      lyr[k][i] = ex * ex + ey * ey <= r2 ? color : lyr[k][i];
    }
  }
}

// the wire's fourteen capsules as corner pairs: the four verticals, the eight i -> i + 2 edges, the back face's cross
__constant__ unsigned char kWireA[14] = {0, 2, 4, 6, 0, 1, 2, 3, 4, 5, 6, 7, 2, 3};
__constant__ unsigned char kWireB[14] = {1, 3, 5, 7, 2, 3, 4, 5, 6, 7, 0, 1, 5, 4};

// out[c] = W[c] != 0 ? W[c] : (T[c] != 0 ? rhe((3 T[c] + U[c]) / 4) : U[c]) on one channel
__device__ __forceinline__ uint32_t blend1(uint32_t u, uint32_t t, uint32_t w) {
  if (w) return w;
  if (!t) return u;
  const uint32_t s = 3 * t + u, q = s >> 2, r = s & 3;
  return q + (r == 3 ? 1u : (r == 2 ? (q & 1u) : 0u));
}

__global__ __launch_bounds__(kThreads) void box_render_kernel(const ctrlv_box_object* __restrict__ objects, int n_objects,
                                                               const ctrlv_box_frame* __restrict__ frames, int Hs, int Ws,
                                                               int tiles_x, int tiles_y, int cull, uint8_t* __restrict__ out) {
  __shared__ Rec recs[kThreads];
  __shared__ int wave_cnt[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, frame = b / tiles_y;
  // the frame's record, made safe: nothing below reads an object outside [first, first + count) of [0, n_objects)
  const ctrlv_box_frame fr = frames[frame];
  int count = 0;
  if (fr.first >= 0 && fr.first < n_objects) count = imax(0, imin(fr.count, imin(n_objects - fr.first, kMaxCount)));
  const bool traj = fr.kind == 1;
  // the tile's pixels that exist, and this lane's 4 x 4 of them
  const int X0 = tx * kTileW, Y0 = ty * kTileH, X1 = imin(X0 + kTileW, Ws) - 1, Y1 = imin(Y0 + kTileH, Hs) - 1;
  const int qx = X0 + 4 * (tid & 31), qy = Y0 + 4 * (tid >> 5);
  uint32_t U[4][4], T[4][4], W[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) U[k][i] = T[k][i] = W[k][i] = 0;

  for (int base = 0; base < count; base += kThreads) {
    // ---- cull and compact one round, in table order
    Rec r;
    bool keep = false;
    if (base + tid < count) {
      const ctrlv_box_object o = objects[fr.first + base + tid];
      const int x1 = clampc(o.x1), x2 = clampc(o.x2), y1 = clampc(o.y1), y2 = clampc(o.y2);
      r.xa = imin(x1, x2); r.xb = imax(x1, x2); r.ya = imin(y1, y2); r.yb = imax(y1, y2);
      r.fill = o.fill_rgb[0] | (uint32_t)o.fill_rgb[1] << 8 | (uint32_t)o.fill_rgb[2] << 16;
      r.line = o.line_rgb[0] | (uint32_t)o.line_rgb[1] << 8 | (uint32_t)o.line_rgb[2] << 16;
      r.flags = o.flags & (CTRLV_BOX_FILL | CTRLV_BOX_OUTLINE | CTRLV_BOX_WIRE);
      r.pad = 0;
      int wx0 = kClamp, wx1 = -kClamp, wy0 = kClamp, wy1 = -kClamp;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int cx = clampc(o.corner[i][0]), cy = clampc(o.corner[i][1]);
        r.cx[i] = (short)cx; r.cy[i] = (short)cy;
        wx0 = imin(wx0, cx); wx1 = imax(wx1, cx); wy0 = imin(wy0, cy); wy1 = imax(wy1, cy);
      }
      // the extent of what the object draws, grown by 1
      int ex0, ex1, ey0, ey1;
      if (traj) {
        ex0 = r.cx[0] - 21; ex1 = r.cx[0] + 21; ey0 = r.cy[0] - 21; ey1 = r.cy[0] + 21;
        keep = true;
      } else {
        ex0 = ey0 = 1 << 20; ex1 = ey1 = -(1 << 20);
        if (r.flags & (CTRLV_BOX_FILL | CTRLV_BOX_OUTLINE)) { ex0 = r.xa - 2; ex1 = r.xb + 2; ey0 = r.ya - 2; ey1 = r.yb + 2; }
        if (r.flags & CTRLV_BOX_WIRE) { ex0 = imin(ex0, wx0 - 2); ex1 = imax(ex1, wx1 + 2); ey0 = imin(ey0, wy0 - 2); ey1 = imax(ey1, wy1 + 2); }
        keep = r.flags != 0;
      }
      keep = keep && (!cull || (ex0 <= X1 && ex1 >= X0 && ey0 <= Y1 && ey1 >= Y0));
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      const int c = wave_cnt[w];
      off += w < wave ? c : 0;
      total += c;
    }
    if (keep) recs[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
    __syncthreads();
    total = __builtin_amdgcn_readfirstlane(total);

    // ---- the survivors in order onto this lane's pixels
    for (int j = 0; j < total; ++j) {
      const Rec& o = recs[j];
      if (traj) {
        const int cx = o.cx[0], cy = o.cy[0];
        if (qx + 3 < cx - 20 || qx > cx + 20 || qy + 3 < cy - 20 || qy > cy + 20) continue;
        draw_disc(U, o.fill, cx, cy, 400, qx, qy);
        draw_disc(U, o.line, cx, cy, 100, qx, qy);
        continue;
      }
      const uint32_t flags = __builtin_amdgcn_readfirstlane(o.flags);
      const int xa = o.xa, xb = o.xb, ya = o.ya, yb = o.yb;
      if (flags & CTRLV_BOX_OUTLINE) {
        const uint32_t col = o.line;
        draw_capsule(U, col, xa, ya, xb, ya, 4u, qx, qy);
        draw_capsule(U, col, xb, ya, xb, yb, 4u, qx, qy);
        draw_capsule(U, col, xb, yb, xa, yb, 4u, qx, qy);
        draw_capsule(U, col, xa, yb, xa, ya, 4u, qx, qy);
      }
      if (flags & CTRLV_BOX_FILL) {
        const uint32_t col = o.fill;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool iny = qy + k >= ya && qy + k <= yb;
#pragma unroll
          for (int i = 0; i < 4; ++i) T[k][i] = iny && qx + i >= xa && qx + i <= xb ? col : T[k][i];
        }
      }
      if (flags & CTRLV_BOX_WIRE) {
        const uint32_t col = o.line;
        for (int e = 0; e < 14; ++e) {
          const int a = kWireA[e], c = kWireB[e];
          draw_capsule(W, col, o.cx[a], o.cy[a], o.cx[c], o.cy[c], e < 12 ? 4u : 1u, qx, qy);
        }
      }
    }
    __syncthreads();                     // the next round overwrites recs and wave_cnt
  }

  // ---- blend and store: per channel one 32-bit word where the address allows it
  if (qx >= Ws) return;
  const int n = imin(4, Ws - qx);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = qy + k;
    if (y >= Hs) break;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t word = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        word |= blend1((U[k][i] >> (8 * c)) & 255u, (T[k][i] >> (8 * c)) & 255u, (W[k][i] >> (8 * c)) & 255u) << (8 * i);
      uint8_t* p = out + (((size_t)frame * 3 + c) * Hs + y) * Ws + qx;
      if (n == 4 && ((uintptr_t)p & 3) == 0) {
        *(uint32_t*)p = word;
      } else if (n == 4 && ((uintptr_t)p & 1) == 0) {
        ((uint16_t*)p)[0] = (uint16_t)word;
        ((uint16_t*)p)[1] = (uint16_t)(word >> 16);
      } else {
        for (int i = 0; i < n; ++i) p[i] = (uint8_t)(word >> (8 * i));
      }
    }
  }
}

// out = ((float) v / 255 - 0.5) / 0.5, each operation rounded in fp32 (ToTensor, Normalize), then the element rounding.  Four
// values per thread: one 32-bit load where the source is aligned, one 16- or 8-byte store (out is 16-byte aligned).
template <bool F32>
__global__ __launch_bounds__(kThreads) void box_cond_norm_kernel(const uint8_t* __restrict__ src, size_t n, void* __restrict__ out,
                                                                  int src_aligned) {
  const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x, e0 = g * 4;
  if (e0 >= n) return;
  const int m = n - e0 < 4 ? (int)(n - e0) : 4;
  uint32_t word = 0;
  if (m == 4 && src_aligned) {
    word = *(const uint32_t*)(src + e0);
  } else {
    for (int i = 0; i < m; ++i) word |= (uint32_t)src[e0 + i] << (8 * i);
  }
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    v[i] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)((word >> (8 * i)) & 255u), 255.0f), 0.5f), 0.5f);
  if (F32) {
    float* o = (float*)out + e0;
    if (m == 4) {
      *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int i = 0; i < m; ++i) o[i] = v[i];
    }
  } else {
    el_t* o = (el_t*)out + e0;
    if (m == 4) {
      *(uint2*)o = make_uint2(pack_elx2(v[0], v[1]), pack_elx2(v[2], v[3]));
    } else {
      for (int i = 0; i < m; ++i) o[i] = f32_to_el(v[i]);
    }
  }
}

constexpr int kBilinear = 2;      // PIL's code, as ctrlv_resize_frames_u8 takes it

int render_check(const void* objects, int n_objects, const void* frames, int n_frames, int Hs, int Ws) {
  CTRLV_CHECK_ARG(objects != nullptr && frames != nullptr, "render_box_frames: the object / frame table is null (device pointers)");
  CTRLV_CHECK_ARG(n_objects >= 0, "render_box_frames: n_objects=%d is negative", n_objects);
  CTRLV_CHECK_SHAPE(n_frames >= 1, "render_box_frames: n_frames=%d must be >= 1", n_frames);
  CTRLV_CHECK_SHAPE(Hs >= 1 && Ws >= 1 && Hs <= kMaxSide && Ws <= kMaxSide, "render_box_frames: source size %d x %d must be in "
                    "[1, %d] per axis", Hs, Ws, kMaxSide);
  const long long tiles = (long long)((Ws + kTileW - 1) / kTileW) * ((Hs + kTileH - 1) / kTileH) * n_frames;
  CTRLV_CHECK_SHAPE(tiles <= 2147483647ll, "render_box_frames: %d frames of %d x %d are %lld tiles, more than 2^31 - 1", n_frames, Hs,
                    Ws, tiles);
  return CTRLV_OK;
}

struct CondLayout {          // ctrlv_box_frames_cond's workspace
  bool resize;
  size_t render, resized, resize_ws, resize_bytes, total;
};

// the sizes of one ctrlv_box_frames_cond call; own_u8: the caller gives out_u8, the render does not live in ws
int cond_layout(int n_frames, int Hs, int Ws, int H, int W, bool own_u8, CondLayout* L) {
  CTRLV_CHECK_SHAPE(n_frames >= 1 && n_frames <= 2147483647 / 3, "box_frames_cond: n_frames=%d", n_frames);
  CTRLV_CHECK_SHAPE(Hs >= 1 && Ws >= 1 && Hs <= kMaxSide && Ws <= kMaxSide, "box_frames_cond: source size %d x %d must be in "
                    "[1, %d] per axis", Hs, Ws, kMaxSide);
  CTRLV_CHECK_SHAPE(H >= 1 && W >= 1, "box_frames_cond: working size %d x %d", H, W);
  L->resize = Hs != H || Ws != W;
  size_t o = 0;
  L->render = o;
  if (!own_u8) o += up256((size_t)n_frames * 3 * Hs * Ws);
  L->resized = L->resize_ws = o;
  L->resize_bytes = 0;
  if (L->resize) {
    L->resize_bytes = ctrlv_resize_frames_ws_bytes(3 * n_frames, Hs, Ws, H, W, kBilinear);
    if (L->resize_bytes == 0) return CTRLV_E_BAD_SHAPE;            // (the resize has named its refusal)
    o += up256((size_t)n_frames * 3 * H * W);
    L->resize_ws = o;
    o += up256(L->resize_bytes);
  }
  L->total = o > 0 ? o : 256;
  return CTRLV_OK;
}

uint32_t mulhi(uint32_t a, uint32_t b, uint32_t* lo) {
  const uint64_t p = (uint64_t)a * b;
  *lo = (uint32_t)p;
  return (uint32_t)(p >> 32);
}

// Philox4x32-10 on the host (ctrlv_randn's generator: csrc/philox.h has the device form)
void philox_host(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* x) {
  for (int r = 0; r < 10; ++r) {
    uint32_t lo0, lo1;
    const uint32_t hi0 = mulhi(0xD2511F53u, c0, &lo0), hi1 = mulhi(0xCD9E8D57u, c2, &lo1);
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

}  // namespace

// What the one-call driver (csrc/pipeline.hip) asks before its first launch: every refusal of ctrlv_box_frames_cond that depends on
// neither `out` nor the workspace, and the bytes of workspace the call needs without an out_u8.  Not part of the C ABI.
int ctrlv_box_frames_cond_check(const void* objects, int n_objects, const void* frames, int n_frames, int Hs, int Ws, int H, int W,
                                size_t* ws_bytes) {
  CTRLV_TRY(render_check(objects, n_objects, frames, n_frames, Hs, Ws));
  CondLayout L;
  CTRLV_TRY(cond_layout(n_frames, Hs, Ws, H, W, false, &L));
  *ws_bytes = L.total;
  return CTRLV_OK;
}

extern "C" int ctrlv_render_box_frames(const ctrlv_box_object* objects, int n_objects, const ctrlv_box_frame* frames, int n_frames,
                                       int Hs, int Ws, void* out_u8, ctrlv_stream_t stream) {
  CTRLV_TRY(render_check(objects, n_objects, frames, n_frames, Hs, Ws));
  CTRLV_CHECK_ARG(out_u8 != nullptr, "render_box_frames: out_u8 is null");
  const int tiles_x = (Ws + kTileW - 1) / kTileW, tiles_y = (Hs + kTileH - 1) / kTileH;
  // developer switch, read at every call so that one process can alternate the two arms (tools/box_render_bench.py):
  // CTRLV_BOX_CULL=0 makes every tile walk every object of its frame -- the walk without binning, same bytes -- to price the binning
  const char* env = getenv("CTRLV_BOX_CULL");
  const int cull = env && env[0] == '0' ? 0 : 1;
  box_render_kernel<<<dim3((unsigned)(tiles_x * tiles_y * n_frames)), dim3(kThreads), 0, (hipStream_t)stream>>>(
      objects, n_objects, frames, Hs, Ws, tiles_x, tiles_y, cull, (uint8_t*)out_u8);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" size_t ctrlv_box_frames_cond_ws_bytes(int n_frames, int Hs, int Ws, int H, int W) {
  CondLayout L;
  return cond_layout(n_frames, Hs, Ws, H, W, false, &L) == CTRLV_OK ? L.total : 0;
}

extern "C" int ctrlv_box_frames_cond(const ctrlv_box_object* objects, int n_objects, const ctrlv_box_frame* frames, int n_frames,
                                     int Hs, int Ws, int H, int W, void* out, int out_dtype, void* out_u8, void* ws, size_t ws_bytes,
                                     ctrlv_stream_t stream) {
  CTRLV_TRY(render_check(objects, n_objects, frames, n_frames, Hs, Ws));
  CondLayout L;
  CTRLV_TRY(cond_layout(n_frames, Hs, Ws, H, W, out_u8 != nullptr, &L));
  CTRLV_CHECK_ARG(out != nullptr && ((uintptr_t)out & 15) == 0, "box_frames_cond: out must be non-null and 16-byte aligned");
  CTRLV_CHECK_DTYPE(out_dtype == 0 || out_dtype == CTRLV_ELEM_DTYPE, "box_frames_cond: out_dtype code %d (0 fp32 or %d, this "
                    "library's element type)", out_dtype, CTRLV_ELEM_DTYPE);
  CTRLV_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 15) == 0, "box_frames_cond: the workspace must be non-null and 16-byte aligned");
  if (ws_bytes < L.total) {
    ctrlv_set_error("box_frames_cond: ws_bytes=%zu is smaller than the %zu bytes this call needs (ctrlv_box_frames_cond_ws_bytes)",
                    ws_bytes, L.total);
    return CTRLV_E_WORKSPACE;
  }
  char* base = (char*)ws;
  uint8_t* render = out_u8 ? (uint8_t*)out_u8 : (uint8_t*)(base + L.render);
  CTRLV_TRY(ctrlv_render_box_frames(objects, n_objects, frames, n_frames, Hs, Ws, render, stream));
  const uint8_t* src = render;
  if (L.resize) {
    CTRLV_TRY(ctrlv_resize_frames_u8(render, 3 * n_frames, Hs, Ws, base + L.resized, H, W, kBilinear, base + L.resize_ws,
                                     L.resize_bytes, stream));
    src = (const uint8_t*)(base + L.resized);
  }
  const size_t n = (size_t)n_frames * 3 * H * W, groups = (n + 3) / 4, blocks = (groups + kThreads - 1) / kThreads;
  CTRLV_CHECK_SHAPE(blocks <= 2147483647ull, "box_frames_cond: %zu output values", n);
  const int aligned = ((uintptr_t)src & 3) == 0;
  if (out_dtype == 0)
    box_cond_norm_kernel<true><<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(src, n, out, aligned);
  else
    box_cond_norm_kernel<false><<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(src, n, out, aligned);
  CTRLV_LAUNCH_CHECK();
  return CTRLV_OK;
}

extern "C" int ctrlv_box_class_color(int id, uint8_t* rgb) {
  // plotting.py:30 TYPE_LOOKUP: BLUE, WHITE, RED, YELLOW, PURPLE, BROWN, GREEN, ORANGE, LIGHTPURPLE, LIGHTRED, GRAY
  static const uint8_t kPalette[11][3] = {{255, 0, 0},   {255, 255, 255}, {0, 0, 255},     {2, 255, 250},   {247, 44, 200}, {42, 42, 165},
                                          {0, 255, 0},   {44, 162, 247},  {255, 153, 204}, {204, 204, 255}, {128, 128, 128}};
  CTRLV_CHECK_ARG(rgb != nullptr, "box_class_color: rgb is null");
  CTRLV_CHECK_ARG(id >= 0 && id < 11, "box_class_color: id=%d is outside the palette's [0, 11)", id);
  for (int c = 0; c < 3; ++c) rgb[c] = kPalette[id][c];
  return CTRLV_OK;
}

extern "C" int ctrlv_box_track_color(uint64_t seed, int64_t track_id, uint8_t* rgb) {
  CTRLV_CHECK_ARG(rgb != nullptr, "box_track_color: rgb is null");
  uint32_t x[4];
  const uint64_t t = (uint64_t)track_id;
  philox_host((uint32_t)t, (uint32_t)(t >> 32), 7u, 0u, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), x);
  for (int c = 0; c < 3; ++c) rgb[c] = (uint8_t)(50u + (uint32_t)(((uint64_t)x[c] * 205u) >> 32));
  return CTRLV_OK;
}

extern "C" int ctrlv_box_project_corners(const double* cam_to_img, int cols, const double* location, const double* dimensions,
                                         double rot_y, int16_t* corners) {
#pragma clang fp contract(off)
  CTRLV_CHECK_ARG(cam_to_img != nullptr && location != nullptr && dimensions != nullptr && corners != nullptr,
                  "box_project_corners: null pointer");
  CTRLV_CHECK_SHAPE(cols == 3 || cols == 4, "box_project_corners: cols=%d must be 3 or 4", cols);
  const double pi = 3.141592653589793;
  const double ca = cos(-rot_y + pi / 2), cb = cos(-rot_y), sa = sin(-rot_y + pi / 2), sb = sin(-rot_y);
  int n = 0;
  for (int i = 1; i >= -1; i -= 2)
    for (int j = 1; j >= -1; j -= 2)
      for (int k = 0; k <= 1; ++k, ++n) {
        double pt[4];
        pt[0] = location[0] + i * dimensions[1] / 2 * ca + (j * i) * dimensions[2] / 2 * cb;
        pt[2] = location[2] + i * dimensions[1] / 2 * sa + (j * i) * dimensions[2] / 2 * sb;
        pt[1] = location[1] - k * dimensions[0];
        pt[3] = 1.0;
        double v[3];
        for (int r = 0; r < 3; ++r) {
          double s = 0.0;
          for (int c = 0; c < cols; ++c) s += cam_to_img[r * cols + c] * pt[c];
          v[r] = s;
        }
        const double den = fabs(v[2]) > 1e-4 ? v[2] : 1e-4;
        for (int a = 0; a < 2; ++a) {
          const double u = v[a] / den;
          // truncation toward zero, then the clamp (the comparisons are false for a NaN: it becomes 0)
          corners[2 * n + a] = u >= (double)kClamp ? (int16_t)kClamp : (u <= -(double)kClamp ? (int16_t)-kClamp : (u == u ? (int16_t)(int)u : (int16_t)0));
        }
      }
  return CTRLV_OK;
}
