// Window attention: what the VALU kernels and the host entry points (winattn.hip) share with the matrix-core
// kernels (winattn_mfma.hip) -- the descriptor every kernel takes, its validation, the shape of a family's launch plan,
// and the window / token geometry on the device.
#pragma once
#include "icm_common.h"

namespace icm {

struct WaDesc {
  const float* qkv;
  const float* table;
  float* out;          // fwd
  const float* dout;   // bwd
  float* dqkv;         // bwd
  float* dtable_ws;    // bwd: partial tables [slab][heads][(2ws-1)^2], slab = window (4x4 matrix cores: group of four)
  int N, C, H, W, heads, shift, nwx, nwy;
  float scale;
  int ngx;             // groups of four windows per row (the 4x4 matrix-core kernels' wave task)
  int ws, hd, T, G;    // window size and head dim are template or literal in the matrix-core kernels
};

// The one place a geometry is checked: ICM_ERR_ARG for what the reference would raise on, ICM_ERR_UNSUPPORTED for
// windows no kernel here serves.  Pointers are the caller's to set.
inline int fill_desc(WaDesc& d, int N, int C, int H, int W, int heads, int ws, int shift) {
  if (N <= 0 || C <= 0 || heads <= 0 || C % heads != 0 || ws <= 0) return ICM_ERR_ARG;
  if (shift < 0 || shift >= ws) return ICM_ERR_ARG;            // assert at win_attention.py:144
  if (H % ws != 0 || W % ws != 0) return ICM_ERR_ARG;          // view() would raise in window_partition
  if (ws * ws > 64) return ICM_ERR_UNSUPPORTED;
  d.N = N; d.C = C; d.H = H; d.W = W; d.heads = heads; d.ws = ws; d.shift = shift; d.hd = C / heads;
  d.T = ws * ws; d.nwx = W / ws; d.nwy = H / ws;
  d.G = 64 / d.T;   // heads per wave of the VALU kernels (1 for 8x8 windows, 4 for 4x4)
  d.ngx = (d.nwx + 3) / 4;
  d.scale = 1.0f / sqrtf((float)d.hd);
  return ICM_OK;
}

// How one kernel family serves a checked geometry in one direction
struct WaPlan {
  void (*fn)(const WaDesc);
  int grid, block;
  size_t lds;
  int slabs;   // table-gradient slabs the backward writes
};
// A family's plan: ICM_OK and p filled when the family takes d, else ICM_ERR_UNSUPPORTED (window size, a head dim
// outside its table, more LDS than a workgroup may ask for).  Pure host code, no HIP call.
typedef int (*WaPlanFn)(const WaDesc& d, int backward, WaPlan& p);
constexpr size_t kWaLdsLimit = 160 * 1024;
int winattn_mfma_plan(const WaDesc& d, int backward, WaPlan& p);     // 8x8 windows on the matrix cores
int winattn_mfma16_plan(const WaDesc& d, int backward, WaPlan& p);   // 4x4 windows on the matrix cores

__device__ __forceinline__ int region(int s, int L, int ws, int shift) {
  return s < L - ws ? 0 : (s < L - shift ? 1 : 2);
}

// Per-token geometry of token j of window (wy, wx); ws is d.ws, passed so that a literal folds the divisions
struct Tok {
  int pix;   // oy*W + ox in the original (un-shifted) image
  int lab;   // shift-mask region label
  int r, c;  // row / col inside the window
};
__device__ __forceinline__ Tok token(const WaDesc& d, int ws, int wy, int wx, int j) {
  Tok t;
  t.r = j / ws;
  t.c = j - t.r * ws;
  const int sy = wy * ws + t.r, sx = wx * ws + t.c;
  int oy = sy + d.shift, ox = sx + d.shift;
  if (oy >= d.H) oy -= d.H;
  if (ox >= d.W) ox -= d.W;
  t.pix = oy * d.W + ox;
  t.lab = d.shift > 0 ? region(sy, d.H, ws, d.shift) * 3 + region(sx, d.W, ws, d.shift) : 0;
  return t;
}

}  // namespace icm
