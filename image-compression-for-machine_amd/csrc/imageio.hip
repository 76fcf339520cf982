// The 8-bit image boundary of the codec on the device, gfx950: what torchvision's ToTensor + F.pad do before compress()
// and what crop + clamp + ToPILImage do after decompress(), so that an image crosses PCIe as bytes and the padded f32
// planes are written / read once.
//
//   image_u8_to_f32_kernel   interleaved [H, W, 3] bytes -> planar [3, OH, OW] f32, image at (top, left), +0.0 around it
//   image_batch_u8_to_f32_kernel   the same conversion for a training batch: B crop windows cut out of an arena of
//                            images (icm_crop_desc each) -> planar [B, 3, CH, CW] f32, +0.0 outside the image
//   image_f32_to_u8_kernel   planar [3, PH, PW] f32 -> interleaved [H, W, 3] bytes of the window at (top, left);
//                            with a reference image also one partial sum of squared byte differences per workgroup
//   image_sse_finish_kernel  adds the partial sums (64-bit integers: exact, whatever the order)
//   image_tile_blend_kernel  adds one decoded tile's window, weighted by its seam ramps, into the f32 canvas of a
//                            tiled image (planar [3, PH, PW] -> planar [3, H, W]); a thread owns four pixels of a row
//   image_cell_stats_kernel  interleaved [H, W, 3] bytes -> (n, sum Y, sum Y^2) of the integer luma over every 16 x 16
//                            cell of the padded image's grid (the encoder's variance-adaptive quality maps)
//
// Pure bandwidth work.  A thread owns a run of 16 pixels of one row: 48 interleaved bytes = three 16-byte accesses,
// and 16 floats = four 16-byte accesses in each of the three planes.  Whether the 16-byte form may be used is decided
// per run and per side (the run lies wholly inside the row and its first byte is 16-byte aligned); every other run --
// row ends, widths that are not multiples of 16, odd pointers -- moves its pixels one at a time through the same
// registers.  No scratch, no atomics.
//
// Values.  v / 255 must be the correctly rounded f32 quotient (ToTensor divides on the host); it is read from a
// 256-entry table that the host compiler evaluates (IEEE division at compile time), staged in LDS once per workgroup.
// The way back is clamp to [0, 1], one f32 multiplication by 255 (correctly rounded on every target) and truncation.
// NaN input to image_f32_to_u8 is unspecified.
#include "icm_common.h"
#include "image_u8.h"

namespace {

using icm::quantise_u8;   // clamp(0, 1).mul(255).to(uint8): image_u8.h

constexpr int RUN = 16;        // pixels per thread
constexpr int BLOCK = 256;
constexpr int MAX_SIDE = 32768;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct U8Table {
  float v[256];
};
constexpr U8Table make_u8_table() {
  U8Table t{};
  for (int i = 0; i < 256; ++i) t.v[i] = (float)i / 255.0f;
  return t;
}
static_assert(make_u8_table().v[0] == 0.0f && make_u8_table().v[255] == 1.0f && make_u8_table().v[51] == 0.2f, "u8 table");
__device__ const U8Table u8_table = make_u8_table();

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the 48 bytes of a run from three 16-byte loads (p is 16-byte aligned)
__device__ __forceinline__ void load_run16(const uint8_t* p, uint32_t (&w)[12]) {
  const u32x4* q4 = reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const u32x4 t = q4[q];
    w[4 * q] = t[0];
    w[4 * q + 1] = t[1];
    w[4 * q + 2] = t[2];
    w[4 * q + 3] = t[3];
  }
}

// the pixels sx0 .. sx0 + 15 of a row of W pixels, one byte at a time; pixels outside the row stay zero bytes
__device__ __forceinline__ void gather_run(const uint8_t* row, int sx0, int W, uint32_t (&w)[12]) {
#pragma unroll
  for (int px = 0; px < RUN; ++px) {
    const int sx = sx0 + px;
    if ((unsigned)sx < (unsigned)W) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int b = 3 * px + c;
        w[b >> 2] |= (uint32_t)row[(size_t)sx * 3 + c] << (8 * (b & 3));
      }
    }
  }
}

// the 48 bytes of a run that starts at p, whatever its byte residue, through the dword-aligned window around them (the
// access image_batch_u8_to_f32_kernel describes and spells out in its own body).  The window may begin up to 3 bytes
// before the run and end up to 3 bytes after it, so it is read only for a run that lies inside its row (in_row) and
// whose window lies inside the image's bytes [img, end); false, and w untouched, otherwise
__device__ __forceinline__ bool load_run_window(bool in_row, const uint8_t* p, const uint8_t* img, const uint8_t* end,
                                                uint32_t (&w)[12]) {
  const uint32_t res = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
  const uint32_t* a = reinterpret_cast<const uint32_t*>(p - res);
  if (in_row && reinterpret_cast<const uint8_t*>(a) >= img &&
      reinterpret_cast<const uint8_t*>(a) + (res ? 52 : 48) <= end) {
    uint32_t t[13];
#pragma unroll
    for (int k = 0; k < 12; ++k) t[k] = a[k];
    t[12] = res ? a[12] : 0u;
#pragma unroll
    for (int k = 0; k < 12; ++k) w[k] = __builtin_amdgcn_alignbyte(t[k + 1], t[k], res);
    return true;
  }
  return false;
}

// a run's 48 interleaved bytes -> 16 floats in each of the three planes, out = the run's first element of plane 0.
// dvec: OW % 4 == 0 and a 16-byte aligned dst (host-checked), so every group of four floats at a column that is a
// multiple of four lies wholly inside the row and is 16-byte aligned
__device__ __forceinline__ void store_run(const float* lut, const uint32_t (&w)[12], float* out, size_t plane, int ox0,
                                          int OW, int dvec) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = 3 * (4 * q + j) + c;
        v[j] = lut[(w[b >> 2] >> (8 * (b & 3))) & 255u];
      }
      float* o = out + c * plane + 4 * q;
      const int ox = ox0 + 4 * q;
      if (dvec) {
        if (ox < OW) *reinterpret_cast<f32x4*>(o) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ox + j < OW) o[j] = v[j];
      }
    }
  }
}

__global__ __launch_bounds__(BLOCK) void image_u8_to_f32_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                                 float* __restrict__ dst, int OH, int OW, int top,
                                                                 int left, int runs_per_row, long long total_runs,
                                                                 int dvec) {
  __shared__ float lut[256];
  lut[threadIdx.x] = u8_table.v[threadIdx.x];
  __syncthreads();
  const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= total_runs) return;
  const int oy = (int)(g / runs_per_row);
  const int ox0 = ((int)(g - (long long)oy * runs_per_row)) * RUN;
  const int sy = oy - top, sx0 = ox0 - left;

  uint32_t w[12];   // the run's 48 interleaved bytes, little-endian words; pixels outside the image are zero bytes
#pragma unroll
  for (int k = 0; k < 12; ++k) w[k] = 0u;
  if ((unsigned)sy < (unsigned)H && sx0 + RUN > 0 && sx0 < W) {
    const uint8_t* row = src + ((size_t)sy * W) * 3;
    if (sx0 >= 0 && sx0 + RUN <= W && aligned16(row + (size_t)sx0 * 3))
      load_run16(row + (size_t)sx0 * 3, w);
    else
      gather_run(row, sx0, W, w);
  }
  store_run(lut, w, dst + (size_t)oy * OW + ox0, (size_t)OH * OW, ox0, OW, dvec);
}

// Batch of crops out of an arena of images: block-uniform sample b, one thread per run of 16 output pixels.  The
// window's x0 is arbitrary, so the 48 source bytes of a run start at any byte residue and a 16-byte aligned access is
// the exception.  A run that lies wholly inside its image row reads the dword-aligned window around its bytes -- 12
// dwords, 13 when the residue mod 4 is not zero, which need dword alignment only and which the compiler merges into
// three 16-byte loads and one dword load -- and moves the bytes down by the residue with one v_alignbyte per word.  The
// window may begin up to 3 bytes before the run and end up to 3 bytes after it, so it is used only where it lies inside
// [image, image + 3 H W): a first or last run of an image that fails this, and every run that crosses a row end,
// takes the byte path.
__global__ __launch_bounds__(BLOCK) void image_batch_u8_to_f32_kernel(const uint8_t* __restrict__ arena,
                                                                       const icm_crop_desc* __restrict__ desc,
                                                                       float* __restrict__ dst, int CH, int CW,
                                                                       int runs_per_row, int runs_per_image,
                                                                       int blocks_per_image, int dvec) {
  __shared__ float lut[256];
  lut[threadIdx.x] = u8_table.v[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.x / blocks_per_image;
  const int r = (blockIdx.x - b * blocks_per_image) * BLOCK + threadIdx.x;
  if (r >= runs_per_image) return;
  const icm_crop_desc d = desc[b];
  const int oy = r / runs_per_row;
  const int ox0 = (r - oy * runs_per_row) * RUN;
  const int sy = d.y0 + oy, sx0 = d.x0 + ox0;

  uint32_t w[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) w[k] = 0u;
  if ((unsigned)sy < (unsigned)d.H && sx0 + RUN > 0 && sx0 < d.W) {
    const uint8_t* img = arena + d.offset;
    const uint8_t* row = img + ((size_t)sy * d.W) * 3;
    const uint8_t* p = row + (size_t)sx0 * 3;
    const uint32_t res = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(p - res);
    const uint8_t* end = img + (size_t)d.H * d.W * 3;
    if (sx0 >= 0 && sx0 + RUN <= d.W && reinterpret_cast<const uint8_t*>(a) >= img &&
        reinterpret_cast<const uint8_t*>(a) + (res ? 52 : 48) <= end) {
      uint32_t t[13];
#pragma unroll
      for (int k = 0; k < 12; ++k) t[k] = a[k];
      t[12] = res ? a[12] : 0u;
#pragma unroll
      for (int k = 0; k < 12; ++k) w[k] = __builtin_amdgcn_alignbyte(t[k + 1], t[k], res);
    } else {
      gather_run(row, sx0, d.W, w);
    }
  }
  const size_t plane = (size_t)CH * CW;
  store_run(lut, w, dst + (size_t)b * 3 * plane + (size_t)oy * CW + ox0, plane, ox0, CW, dvec);
}

__global__ __launch_bounds__(BLOCK) void image_f32_to_u8_kernel(const float* __restrict__ src, int PH, int PW, int top,
                                                                 int left, uint8_t* __restrict__ dst, int H, int W,
                                                                 const uint8_t* __restrict__ ref,
                                                                 unsigned long long* __restrict__ part,
                                                                 int runs_per_row, long long total_runs) {
  __shared__ unsigned long long red[BLOCK / 64];
  const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
  uint32_t sse = 0u;   // 48 squared differences of at most 255^2 each
  if (g < total_runs) {
    const int y = (int)(g / runs_per_row);
    const int x0 = ((int)(g - (long long)y * runs_per_row)) * RUN;
    const bool full = x0 + RUN <= W;
    const size_t plane = (size_t)PH * PW;
    const float* in = src + (size_t)(top + y) * PW + left + x0;
    const size_t obyte = ((size_t)y * W + x0) * 3;

    uint32_t w[12];   // the run's 48 interleaved output bytes
#pragma unroll
    for (int k = 0; k < 12; ++k) w[k] = 0u;
    // the three planes start a multiple of PH * PW floats apart: one alignment test serves them only if that is a
    // multiple of four, so each plane is tested
    if (full && aligned16(in) && aligned16(in + plane) && aligned16(in + 2 * plane)) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(in + c * plane + 4 * q);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int b = 3 * (4 * q + j) + c;
            w[b >> 2] |= quantise_u8(v[j]) << (8 * (b & 3));
          }
        }
      }
    } else {
#pragma unroll
      for (int px = 0; px < RUN; ++px) {
        if (x0 + px < W) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int b = 3 * px + c;
            w[b >> 2] |= quantise_u8(in[c * plane + px]) << (8 * (b & 3));
          }
        }
      }
    }

    if (ref) {
      uint32_t r[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) r[k] = w[k];   // pixels beyond the row end: equal bytes, no contribution
      if (full && aligned16(ref + obyte)) {
        const u32x4* p = reinterpret_cast<const u32x4*>(ref + obyte);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const u32x4 t = p[q];
          r[4 * q] = t[0];
          r[4 * q + 1] = t[1];
          r[4 * q + 2] = t[2];
          r[4 * q + 3] = t[3];
        }
      } else {
#pragma unroll
        for (int px = 0; px < RUN; ++px) {
          if (x0 + px < W) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int b = 3 * px + c, sh = 8 * (b & 3);
              r[b >> 2] = (r[b >> 2] & ~(255u << sh)) | ((uint32_t)ref[obyte + b] << sh);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 12; ++k) {
#pragma unroll
        for (int s = 0; s < 32; s += 8) {
          const int d = (int)((w[k] >> s) & 255u) - (int)((r[k] >> s) & 255u);
          sse += (uint32_t)(d * d);
        }
      }
    }

    if (full && aligned16(dst + obyte)) {
      u32x4* p = reinterpret_cast<u32x4*>(dst + obyte);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const u32x4 t = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
        p[q] = t;
      }
    } else {
#pragma unroll
      for (int px = 0; px < RUN; ++px) {
        if (x0 + px < W) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int b = 3 * px + c;
            dst[obyte + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
          }
        }
      }
    }
  }

  if (ref) {   // kernel-uniform: every thread of the workgroup reaches the barrier
    unsigned long long s = sse;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// one workgroup: thread t adds partials t, t + 256, ... in index order, then the 256 sums are added in a fixed tree
__global__ __launch_bounds__(BLOCK) void image_sse_finish_kernel(const unsigned long long* __restrict__ part, int n,
                                                                  long long* __restrict__ out) {
  __shared__ unsigned long long red[BLOCK / 64];
  unsigned long long s = 0ull;
  for (int i = threadIdx.x; i < n; i += BLOCK) s += part[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = (long long)((red[0] + red[1]) + (red[2] + red[3]));
}

// Tile assembly of a tiled image: canvas[c][y0 + y][x0 + x] += (wy(y) * wx(x)) * src[c][top + y][left + x] over the
// h x w window.  w?(i) is ramp[i] within m pixels of a side that has a neighbour (ramp[n - 1 - i] at the far side) and 1
// elsewhere; where both bands reach a pixel the near (left / top) side decides.  The two products and the sum are
// single IEEE operations in that association (no contraction into an FMA), so a host restatement agrees bit for bit
// and a pixel under one tile keeps 0 + 1 * v = v.  A thread owns BLEND_RUN adjacent pixels of one row in all three
// planes and shares the weights among them; each side (source, canvas) of each plane moves as one 16-byte access when
// its address is 16-byte aligned and the run lies inside the window, and float by float otherwise.  Plane offsets are
// 64-bit: the canvas of a large image exceeds 2^31 elements.
constexpr int BLEND_RUN = 4;
constexpr int EDGE_LEFT = ICM_TILE_EDGE_LEFT, EDGE_RIGHT = ICM_TILE_EDGE_RIGHT, EDGE_TOP = ICM_TILE_EDGE_TOP,
              EDGE_BOTTOM = ICM_TILE_EDGE_BOTTOM;

// One rounding each, never fused: the headers' __fmul_rn / __fadd_rn are a plain * and + that carry the contraction
// flag of their own translation context, and hipcc folds a pair of them into v_pk_fma_f32.  The same operators under
// contract(off) stay a v_mul / v_add pair.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

__device__ __forceinline__ float blend_weight(const float* __restrict__ ramp, int i, int n, int m, bool near, bool far) {
  if (near && i < m) return ramp[i];
  if (far && n - 1 - i < m) return ramp[n - 1 - i];
  return 1.0f;
}

__global__ __launch_bounds__(BLOCK) void image_tile_blend_kernel(const float* __restrict__ src, int PH, int PW, int top,
                                                                  int left, int h, int w, float* __restrict__ canvas,
                                                                  int H, int W, int y0, int x0,
                                                                  const float* __restrict__ ramp, int m, int edges,
                                                                  int runs_per_row, long long total_runs) {
  const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= total_runs) return;
  const int y = (int)(g / runs_per_row);
  const int x = ((int)(g - (long long)y * runs_per_row)) * BLEND_RUN;
  const bool full = x + BLEND_RUN <= w;

  const float wy = blend_weight(ramp, y, h, m, edges & EDGE_TOP, edges & EDGE_BOTTOM);
  float k[BLEND_RUN];   // wy * wx of the run's pixels
#pragma unroll
  for (int j = 0; j < BLEND_RUN; ++j) {
    const float wx = x + j < w ? blend_weight(ramp, x + j, w, m, edges & EDGE_LEFT, edges & EDGE_RIGHT) : 1.0f;
    k[j] = mul_rn(wy, wx);
  }

  const size_t splane = (size_t)PH * PW, cplane = (size_t)H * W;
  const float* in = src + (size_t)(top + y) * PW + left + x;
  float* out = canvas + (size_t)(y0 + y) * W + x0 + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* ip = in + c * splane;
    float* op = out + c * cplane;
    const bool ovec = full && aligned16(op);
    float s[BLEND_RUN], a[BLEND_RUN];
    if (full && aligned16(ip)) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(ip);
#pragma unroll
      for (int j = 0; j < BLEND_RUN; ++j) s[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < BLEND_RUN; ++j) s[j] = x + j < w ? ip[j] : 0.0f;
    }
    if (ovec) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(op);
#pragma unroll
      for (int j = 0; j < BLEND_RUN; ++j) a[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < BLEND_RUN; ++j) a[j] = x + j < w ? op[j] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < BLEND_RUN; ++j) a[j] = add_rn(a[j], mul_rn(k[j], s[j]));
    if (ovec) {
      const f32x4 v = {a[0], a[1], a[2], a[3]};
      *reinterpret_cast<f32x4*>(op) = v;
    } else {
#pragma unroll
      for (int j = 0; j < BLEND_RUN; ++j)
        if (x + j < w) op[j] = a[j];
    }
  }
}

// Luma statistics of the 16 x 16 cells of a padded image's grid: pixel (y, x) lies in cell ((top + y) / 16,
// (left + x) / 16), Y = (77 R + 150 G + 29 B + 128) >> 8, and a cell's (n, s1, s2) = (its image pixels, sum Y, sum Y^2);
// pad pixels are no pixels.  A workgroup takes a strip of STRIP cells of one row of cells: thread t owns the run of 16
// pixels of row t / 16 of cell t % 16, so a wave reads four image rows of 768 contiguous bytes each -- through the
// dword window wherever the run lies inside its row (3 W bytes a row and an arbitrary left: 16-byte alignment is the
// exception, as for the batch crops), byte by byte at the image's edges.  Bytes outside the image stay zero and give
// Y = 0, so only n has to know about them.  The four rows a wave holds of a cell are added by two shuffles, the four
// waves' partials through LDS, and 3 STRIP threads store the strip's 3 STRIP contiguous integers: every entry of stats is
// written once, by plain vector stores.  Integer sums (s2 <= 256 * 255^2 < 2^24): exact in any order.
constexpr int CELL = 16;
constexpr int STRIP = BLOCK / CELL;   // cells per workgroup
static_assert(CELL == RUN && STRIP == 16 && BLOCK == 256, "a thread owns one row of one cell; four waves of four rows");

__global__ __launch_bounds__(BLOCK) void image_cell_stats_kernel(const uint8_t* __restrict__ img, int H, int W, int top,
                                                                  int left, int gw, int strips,
                                                                  int32_t* __restrict__ stats) {
  __shared__ int32_t red[BLOCK / 64][3 * STRIP];
  const int cy = blockIdx.x / strips;
  const int cx0 = (blockIdx.x - cy * strips) * STRIP;
  const int cell = threadIdx.x & (STRIP - 1), r = threadIdx.x / STRIP;
  const int y = cy * CELL + r - top, x0 = (cx0 + cell) * CELL - left;

  uint32_t w[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) w[k] = 0u;
  int n = 0;
  if ((unsigned)y < (unsigned)H && x0 + RUN > 0 && x0 < W) {
    const uint8_t* row = img + ((size_t)y * W) * 3;
    if (load_run_window(x0 >= 0 && x0 + RUN <= W, row + (size_t)x0 * 3, img, img + (size_t)H * W * 3, w)) {
      n = RUN;
    } else {
      gather_run(row, x0, W, w);
      n = min(x0 + RUN, W) - max(x0, 0);
    }
  }
  int s1 = 0, s2 = 0;
#pragma unroll
  for (int px = 0; px < RUN; ++px) {
    uint32_t c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int b = 3 * px + k;
      c[k] = (w[b >> 2] >> (8 * (b & 3))) & 255u;
    }
    const int Y = (int)((77u * c[0] + 150u * c[1] + 29u * c[2] + 128u) >> 8);
    s1 += Y;
    s2 += Y * Y;
  }
#pragma unroll
  for (int m = STRIP; m < 64; m <<= 1) {   // lanes cell, cell + 16, cell + 32, cell + 48: the wave's four rows
    n += __shfl_xor(n, m, 64);
    s1 += __shfl_xor(s1, m, 64);
    s2 += __shfl_xor(s2, m, 64);
  }
  if ((threadIdx.x & 63) < STRIP) {
    int32_t* o = red[threadIdx.x >> 6] + 3 * cell;
    o[0] = n;
    o[1] = s1;
    o[2] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 3 * STRIP && cx0 + (int)threadIdx.x / 3 < gw)
    stats[((size_t)cy * gw + cx0) * 3 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// runs of a rows x cols image and the workgroups that cover them; false = geometry out of range
bool run_grid(int rows, int cols, int& runs_per_row, long long& total_runs, int& blocks) {
  if (rows <= 0 || cols <= 0 || rows > MAX_SIDE || cols > MAX_SIDE) return false;
  runs_per_row = (cols + RUN - 1) / RUN;
  total_runs = (long long)rows * runs_per_row;
  blocks = (int)((total_runs + BLOCK - 1) / BLOCK);
  return true;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" {

int64_t icm_image_workspace_bytes(int H, int W) {
  int rpr, blocks;
  long long total;
  return run_grid(H, W, rpr, total, blocks) ? (int64_t)blocks * 8 : 0;
}

int icm_image_u8_to_f32(const uint8_t* src, int H, int W, float* dst, int OH, int OW, int top, int left, void* stream) {
  int rpr, blocks, srpr, sblocks;
  long long total, stotal;
  if (!src || !dst || top < 0 || left < 0) return ICM_ERR_ARG;
  if (!run_grid(H, W, srpr, stotal, sblocks) || !run_grid(OH, OW, rpr, total, blocks)) return ICM_ERR_ARG;
  if ((long long)top + H > OH || (long long)left + W > OW) return ICM_ERR_ARG;
  const int dvec = OW % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  hipLaunchKernelGGL(image_u8_to_f32_kernel, dim3(blocks), dim3(BLOCK), 0, ST, src, H, W, dst, OH, OW, top, left, rpr,
                     total, dvec);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_image_batch_u8_to_f32(const uint8_t* arena, const icm_crop_desc* desc, int B, float* dst, int CH, int CW,
                              void* stream) {
  int rpr, bpi;
  long long rpi;
  if (!arena || !desc || !dst || B < 1 || !run_grid(CH, CW, rpr, rpi, bpi)) return ICM_ERR_ARG;
  if ((long long)bpi * B > 0x7fffffffLL) return ICM_ERR_ARG;
  const int dvec = CW % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  hipLaunchKernelGGL(image_batch_u8_to_f32_kernel, dim3((unsigned)(bpi * B)), dim3(BLOCK), 0, ST, arena, desc, dst, CH,
                     CW, rpr, (int)rpi, bpi, dvec);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_image_f32_to_u8(const float* src, int PH, int PW, int top, int left, uint8_t* dst, int H, int W,
                        const uint8_t* ref, int64_t* sse, void* ws, int64_t ws_bytes, void* stream) {
  int rpr, blocks, prpr, pblocks;
  long long total, ptotal;
  if (!src || !dst || top < 0 || left < 0) return ICM_ERR_ARG;
  if (!run_grid(H, W, rpr, total, blocks) || !run_grid(PH, PW, prpr, ptotal, pblocks)) return ICM_ERR_ARG;
  if ((long long)top + H > PH || (long long)left + W > PW) return ICM_ERR_ARG;
  if (ref) {
    if (!sse || !ws || ws_bytes < (int64_t)blocks * 8) return ICM_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(sse)) & 7) return ICM_ERR_ARG;
  }
  unsigned long long* part = ref ? static_cast<unsigned long long*>(ws) : nullptr;
  hipLaunchKernelGGL(image_f32_to_u8_kernel, dim3(blocks), dim3(BLOCK), 0, ST, src, PH, PW, top, left, dst, H, W, ref,
                     part, rpr, total);
  ICM_CHECK_LAUNCH();
  if (ref) {
    hipLaunchKernelGGL(image_sse_finish_kernel, dim3(1), dim3(BLOCK), 0, ST, part, blocks, reinterpret_cast<long long*>(sse));
    ICM_CHECK_LAUNCH();
  }
  return ICM_OK;
}

int icm_image_tile_blend(const float* src, int PH, int PW, int top, int left, int h, int w, float* canvas, int H, int W,
                         int y0, int x0, const float* ramp, int m, int edges, void* stream) {
  if (!src || !canvas || top < 0 || left < 0 || y0 < 0 || x0 < 0 || m < 0 || (m > 0 && !ramp)) return ICM_ERR_ARG;
  if (edges < 0 || edges > 15) return ICM_ERR_ARG;
  for (int v : {PH, PW, h, w, H, W})
    if (v <= 0 || v > MAX_SIDE) return ICM_ERR_ARG;
  if ((long long)top + h > PH || (long long)left + w > PW) return ICM_ERR_ARG;   // the window inside src
  if ((long long)y0 + h > H || (long long)x0 + w > W) return ICM_ERR_ARG;       // and inside the canvas
  if (((edges & (EDGE_LEFT | EDGE_RIGHT)) && m > w) || ((edges & (EDGE_TOP | EDGE_BOTTOM)) && m > h)) return ICM_ERR_ARG;
  const int rpr = (w + BLEND_RUN - 1) / BLEND_RUN;
  const long long total = (long long)h * rpr;                                    // <= 32768 * 8192
  hipLaunchKernelGGL(image_tile_blend_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ST, src, PH,
                     PW, top, left, h, w, canvas, H, W, y0, x0, ramp, m, edges, rpr, total);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_image_cell_stats(const uint8_t* img, int H, int W, int top, int left, int gh, int gw, int32_t* stats,
                         void* stream) {
  constexpr int MAX_CELLS = 1 << 26;   // 16 x (a cell index, one strip past the grid) stays an int
  if (!img || !stats || H < 1 || W < 1 || gh < 1 || gw < 1 || top < 0 || left < 0) return ICM_ERR_ARG;
  if (gh > MAX_CELLS || gw > MAX_CELLS) return ICM_ERR_ARG;
  if ((long long)top + H > (long long)CELL * gh || (long long)left + W > (long long)CELL * gw) return ICM_ERR_ARG;
  const int strips = (gw + STRIP - 1) / STRIP;
  if ((long long)gh * strips > 0x7fffffffLL) return ICM_ERR_ARG;
  hipLaunchKernelGGL(image_cell_stats_kernel, dim3((unsigned)(gh * strips)), dim3(BLOCK), 0, ST, img, H, W, top, left, gw,
                     strips, stats);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

}  // extern "C"
