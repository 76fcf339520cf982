// The error-bounded residual layer of the codec on the device, gfx950 (icm_amd/residual.py, ICMR streams; parity
// unpinned: no counterpart in the reference).  x = the original 8-bit image, xhat = what the decoder makes of the base
// stream, both interleaved [H, W, 3] bytes; D = the bound, s = 2 D + 1.
//
//   residual_code_kernel     x, xhat -> q = sign(x - xhat) ((|x - xhat| + D) div s) in plane order [3, H, W], the class of
//                            every 16 x 16-pixel cell (grid anchored at pixel (0, 0)) and, per sample, its cell's class
//   residual_indexes_kernel  the decoder's expansion: classes [gh, gw] -> one class per sample, [3, H, W]
//   residual_apply_kernel    xhat of a window, q -> min(max(xhat + q s, 0), 255), interleaved bytes of the window
//
// The bound is one number for the image (icm_residual_code / icm_residual_apply) or one byte per 16 x 16-pixel cell of
// the same grid (icm_residual_code_map / icm_residual_apply_map, ICME streams).  Each operation has one element body,
// code_cell and apply_run, and two thin kernels that differ in where the bound comes from: a kernel argument, or the
// map -- read once per wave in residual_code_map_kernel, where a wave owns a cell, and once or twice per run in
// residual_apply_map_kernel, where a run of four window pixels may straddle a cell boundary of the image.  A map byte
// above 32 counts as 32 in both, so that the reciprocal below always divides.
//
// Bands.  The decoder's two operations also take buffers that hold a band of every plane instead of the planes: the
// elements [e_lo, e_hi) of the row-major plane, plane c at c (e_hi - e_lo), which is what a region decode has of the
// symbols (icm_residual_indexes_band / icm_residual_apply_band / icm_residual_apply_map_band).  A band starts and ends
// anywhere in a row.  The kernels and element bodies are the same: Band{stride, lo, hi} says where element e of a
// plane lies, and the whole planes are the band [0, H W).
//
// Integer work only, byte-bound: 6 bytes in and 24 out per pixel for the first, 12 out for the second, 15 in and 3 out
// for the third.  A thread owns four adjacent pixels of one row: 12 interleaved bytes = three dword accesses where the
// run lies inside its row and its first byte is dword-aligned, and four int32 per plane = one 16-byte access where its
// first element is 16-byte aligned; every other run -- row ends, widths that are no multiple of four, odd pointers --
// moves byte by byte and element by element through the same registers.  No LDS, no scratch, no atomics.
//
// The division by s is a multiplication: for n = |r| + D <= 287 and s <= 65, (n m) >> 16 with m = 65536 div s + 1 is
// n div s, because the error of m / 65536 against 1 / s is below 1 / 65536 and 287 / 65536 < 1 / 65 (the test suite
// also walks all (n, s)).
#include "icm_common.h"

namespace {

constexpr int RUN = 4;         // pixels per thread
constexpr int BLOCK = 256;
constexpr int MAX_SIDE = 32768;
constexpr int MAX_D = 32;
constexpr int CELL = 16;
constexpr int WAVES = BLOCK / 64;   // cells per workgroup in residual_code_kernel: neighbours in one row of cells

// class thresholds, round(2^(1 + j / 2)): a cell of N coded samples with S = sum |q| has the class
// #{j : 16 S > N T_j} (icm_amd/residual.py THRESHOLDS; the tests compare the two lists through the classes)
constexpr int NTHRESH = 18;
constexpr int THRESH[NTHRESH] = {2, 3, 4, 6, 8, 11, 16, 23, 32, 45, 64, 91, 128, 181, 256, 362, 512, 724};

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool aligned_to(const void* p, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

// the 12 interleaved bytes of the run's pixels that lie inside the row (n of them), little-endian words, zero elsewhere
__device__ __forceinline__ void load_run(const uint8_t* p, bool full, int n, uint32_t (&w)[3]) {
  if (full && aligned_to(p, 4)) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = q[k];
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = 0u;
#pragma unroll
    for (int b = 0; b < 3 * RUN; ++b)
      if (b < 3 * n) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
  }
}

__device__ __forceinline__ int byte_of(const uint32_t (&w)[3], int b) { return (int)((w[b >> 2] >> (8 * (b & 3))) & 255u); }

// four int32 of one plane, n of them inside the row
__device__ __forceinline__ void store_run(int32_t* o, bool full, int n, const int (&v)[RUN]) {
  if (full && aligned_to(o, 16)) {
    const i32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<i32x4*>(o) = t;
  } else {
#pragma unroll
    for (int j = 0; j < RUN; ++j)
      if (j < n) o[j] = v[j];
  }
}

// One wave owns a cell: lane l holds the four pixels 4 (l % 4) .. of row l / 4, so a wave reads the cell's two blocks
// of 16 rows x 48 bytes and the four waves of a workgroup read 192 contiguous bytes of every row.  S is reduced by six
// shuffles; N is known from the geometry.  Lanes of rows and columns past the image load and store nothing and add 0.
// bound(D, magic) gives the cell's D and magic = 65536 div (2 D + 1) + 1, the same in all lanes; it is asked once the
// loads of the cell's bytes are on their way, so that a bound that is itself loaded does not wait alone.
template <class Bound>
__device__ __forceinline__ void code_cell(const uint8_t* __restrict__ x, const uint8_t* __restrict__ xhat, int H, int W,
                                          Bound bound, int gw, int cy, int cx, int lane,
                                          int32_t* __restrict__ symbols, int32_t* __restrict__ indexes,
                                          int32_t* __restrict__ classes) {
  const int y = cy * CELL + (lane >> 2), px0 = cx * CELL + RUN * (lane & 3);
  const int n = y < H ? min(max(W - px0, 0), RUN) : 0;   // the run's pixels inside the image
  const bool full = n == RUN;

  int q[3 * RUN];
  int S = 0;
#pragma unroll
  for (int b = 0; b < 3 * RUN; ++b) q[b] = 0;
  if (n > 0) {
    const size_t o = ((size_t)y * W + px0) * 3;
    uint32_t a[3], e[3];
    load_run(x + o, full, n, a);
    load_run(xhat + o, full, n, e);
    int D, magic;
    bound(D, magic);
#pragma unroll
    for (int b = 0; b < 3 * RUN; ++b) {   // bytes past the row end are zero on both sides: q = 0
      const int r = byte_of(a, b) - byte_of(e, b);
      const int m = ((abs(r) + D) * magic) >> 16;
      q[b] = r < 0 ? -m : m;
      S += m;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) S += __shfl_xor(S, m, 64);
  const int N = 3 * min(CELL, H - cy * CELL) * min(CELL, W - cx * CELL);
  int cls = 0;
#pragma unroll
  for (int j = 0; j < NTHRESH; ++j) cls += 16 * S > N * THRESH[j] ? 1 : 0;   // 16 S <= 2^22, N T <= 2^20

  if (n > 0) {
    const size_t plane = (size_t)H * W, e0 = (size_t)y * W + px0;
    const int k[RUN] = {cls, cls, cls, cls};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v[RUN] = {q[c], q[3 + c], q[6 + c], q[9 + c]};
      store_run(symbols + c * plane + e0, full, n, v);
      store_run(indexes + c * plane + e0, full, n, k);
    }
  }
  if (lane == 0) classes[(size_t)cy * gw + cx] = cls;
}

__global__ __launch_bounds__(BLOCK) void residual_code_kernel(const uint8_t* __restrict__ x,
                                                               const uint8_t* __restrict__ xhat, int H, int W, int D,
                                                               int magic, int gw, int strips,
                                                               int32_t* __restrict__ symbols,
                                                               int32_t* __restrict__ indexes,
                                                               int32_t* __restrict__ classes) {
  const int cy = blockIdx.x / strips;
  const int cx = (blockIdx.x - cy * strips) * WAVES + (threadIdx.x >> 6);
  if (cx >= gw) return;   // wave-uniform; the kernel has no barrier
  code_cell(x, xhat, H, W, [=](int& d, int& m) { d = D; m = magic; }, gw, cy, cx, threadIdx.x & 63, symbols, indexes,
            classes);
}

// the cell's bound from the map: one byte per wave, the same address in all lanes, read first and, when the cell's
// bytes have been asked for, made a scalar so that the division for the reciprocal is done once per wave
__global__ __launch_bounds__(BLOCK) void residual_code_map_kernel(const uint8_t* __restrict__ x,
                                                                   const uint8_t* __restrict__ xhat, int H, int W,
                                                                   const uint8_t* __restrict__ dmap, int gw, int strips,
                                                                   int32_t* __restrict__ symbols,
                                                                   int32_t* __restrict__ indexes,
                                                                   int32_t* __restrict__ classes) {
  const int cy = blockIdx.x / strips;
  const int cx = (blockIdx.x - cy * strips) * WAVES + (threadIdx.x >> 6);
  if (cx >= gw) return;   // wave-uniform; the kernel has no barrier
  const int byte = dmap[(size_t)cy * gw + cx];
  code_cell(x, xhat, H, W, [=](int& d, int& m) {
    d = __builtin_amdgcn_readfirstlane(min(byte, MAX_D));
    m = 65536 / (2 * d + 1) + 1;
  }, gw, cy, cx, threadIdx.x & 63, symbols, indexes, classes);
}

// where the elements of a plane lie in a symbols / indexes buffer: element e of plane c, lo <= e < hi, at
// c stride + e - lo.  The whole planes: {H W, 0, H W}.
struct Band {
  long long stride, lo, hi;
};

// a thread owns four adjacent samples of one row (they share a cell) in the three planes; the rows are those of the
// band, y_first onwards, and the samples of its first and last row that lie outside it are not stored
__global__ __launch_bounds__(BLOCK) void residual_indexes_kernel(const int32_t* __restrict__ classes, int W, int gw,
                                                                  Band band, int y_first,
                                                                  int32_t* __restrict__ indexes, int runs_per_row,
                                                                  long long total_runs) {
  const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= total_runs) return;
  const int yr = (int)(g / runs_per_row);
  const int y = y_first + yr;
  const int x0 = ((int)(g - (long long)yr * runs_per_row)) * RUN;
  const long long e0 = (long long)y * W + x0;
  const int j0 = (int)min(max(band.lo - e0, 0ll), (long long)RUN);             // the run's samples inside the band:
  const int n = (int)max(min(min((long long)(W - x0), band.hi - e0), (long long)RUN), 0ll);   // j0 <= j < n
  if (j0 >= n) return;
  const int cls = classes[(size_t)(y / CELL) * gw + x0 / CELL];
  const int k[RUN] = {cls, cls, cls, cls};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // where the run's first sample would lie: in front of the band, even of the buffer, if j0 > 0 -- an address only,
    // the stores below touch o[j0 .. n - 1] alone, all inside the band
    int32_t* o = indexes + c * band.stride + (e0 - band.lo);
    if (j0 == 0) {
      store_run(o, n == RUN, n, k);
    } else {
#pragma unroll
      for (int j = 0; j < RUN; ++j)
        if (j >= j0 && j < n) o[j] = cls;
    }
  }
}

// a thread owns four adjacent pixels of one row of the window; s[j] is the step 2 D + 1 of pixel j's cell.  |q| >= 256
// saturates whatever s is, so q is clamped to +-256 first and the product stays small: the result is that of the exact
// integers for every int32 q
__device__ __forceinline__ void apply_run(const uint8_t* __restrict__ xhat, const int32_t* __restrict__ symbols,
                                          Band band, int W, int y0, int x0, int w, int y, int x, const int (&s)[RUN],
                                          uint8_t* __restrict__ out) {
  const int n = min(w - x, RUN);
  const bool full = n == RUN;
  const size_t o = ((size_t)y * w + x) * 3;
  uint32_t e[3];
  load_run(xhat + o, full, n, e);

  const long long e0 = (long long)(y0 + y) * W + x0 + x - band.lo;   // the window lies inside the band
  uint32_t r[3] = {0u, 0u, 0u};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int32_t* sp = symbols + c * band.stride + e0;
    int q[RUN];
    if (full && aligned_to(sp, 16)) {
      const i32x4 t = *reinterpret_cast<const i32x4*>(sp);
#pragma unroll
      for (int j = 0; j < RUN; ++j) q[j] = t[j];
    } else {
#pragma unroll
      for (int j = 0; j < RUN; ++j) q[j] = j < n ? sp[j] : 0;
    }
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
      const int b = 3 * j + c;
      const int v = min(max(byte_of(e, b) + min(max(q[j], -256), 256) * s[j], 0), 255);
      r[b >> 2] |= (uint32_t)v << (8 * (b & 3));
    }
  }
  uint8_t* op = out + o;
  if (full && aligned_to(op, 4)) {
    uint32_t* p = reinterpret_cast<uint32_t*>(op);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = r[k];
  } else {
#pragma unroll
    for (int b = 0; b < 3 * RUN; ++b)
      if (b < 3 * n) op[b] = (uint8_t)(r[b >> 2] >> (8 * (b & 3)));
  }
}

__global__ __launch_bounds__(BLOCK) void residual_apply_kernel(const uint8_t* __restrict__ xhat,
                                                                const int32_t* __restrict__ symbols, Band band,
                                                                int W, int y0, int x0, int h, int w, int s,
                                                                uint8_t* __restrict__ out, int runs_per_row,
                                                                long long total_runs) {
  const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= total_runs) return;
  const int y = (int)(g / runs_per_row);
  const int x = ((int)(g - (long long)y * runs_per_row)) * RUN;
  const int sj[RUN] = {s, s, s, s};
  apply_run(xhat, symbols, band, W, y0, x0, w, y, x, sj, out);
}

// The cell of a pixel is that of its image position (y0 + y, x0 + x + j).  The run's pixels inside the window span at
// most two cells of one row of cells (4 <= 16): the first pixel's and the last one's.  Their bytes are read, the second
// only where it is another cell, and every pixel takes the one of its own column.  Both lie inside the map: the window
// lies inside the image.
__global__ __launch_bounds__(BLOCK) void residual_apply_map_kernel(const uint8_t* __restrict__ xhat,
                                                                    const int32_t* __restrict__ symbols, Band band,
                                                                    int W, int y0, int x0, int h, int w,
                                                                    const uint8_t* __restrict__ dmap, int gw,
                                                                    uint8_t* __restrict__ out, int runs_per_row,
                                                                    long long total_runs) {
  const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= total_runs) return;
  const int y = (int)(g / runs_per_row);
  const int x = ((int)(g - (long long)y * runs_per_row)) * RUN;
  const int px = x0 + x, last = px + min(w - x, RUN) - 1;
  const int c0 = px / CELL, c1 = last / CELL;
  const uint8_t* row = dmap + (size_t)((y0 + y) / CELL) * gw;
  const int s0 = 2 * min((int)row[c0], MAX_D) + 1;
  const int s1 = c1 != c0 ? 2 * min((int)row[c1], MAX_D) + 1 : s0;
  int sj[RUN];
#pragma unroll
  for (int j = 0; j < RUN; ++j) sj[j] = (px + j) / CELL == c0 ? s0 : s1;   // pixels past the window are not stored
  apply_run(xhat, symbols, band, W, y0, x0, w, y, x, sj, out);
}

bool side_ok(int v) { return v >= 1 && v <= MAX_SIDE; }

// a band of the planes of an H x W image that is not empty
bool band_ok(int H, int W, int64_t e_lo, int64_t e_hi) { return e_lo >= 0 && e_lo < e_hi && e_hi <= (int64_t)H * W; }

// the window inside the image, and every one of its samples inside the band
bool window_ok(int H, int W, int y0, int x0, int h, int w, int64_t e_lo, int64_t e_hi) {
  if (y0 < 0 || x0 < 0 || (long long)y0 + h > H || (long long)x0 + w > W) return false;
  return (int64_t)y0 * W + x0 >= e_lo && (int64_t)(y0 + h - 1) * W + x0 + w <= e_hi;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" {

int icm_residual_code(const uint8_t* x, const uint8_t* xhat, int H, int W, int D, int32_t* symbols, int32_t* indexes,
                      int32_t* classes, void* stream) {
  if (!x || !xhat || !symbols || !indexes || !classes) return ICM_ERR_ARG;
  if (!side_ok(H) || !side_ok(W) || D < 0 || D > MAX_D) return ICM_ERR_ARG;
  const int gh = (H + CELL - 1) / CELL, gw = (W + CELL - 1) / CELL;
  const int strips = (gw + WAVES - 1) / WAVES;                    // gh strips <= 2048 * 512
  hipLaunchKernelGGL(residual_code_kernel, dim3((unsigned)(gh * strips)), dim3(BLOCK), 0, ST, x, xhat, H, W, D,
                     65536 / (2 * D + 1) + 1, gw, strips, symbols, indexes, classes);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_residual_code_map(const uint8_t* x, const uint8_t* xhat, int H, int W, const uint8_t* dmap, int32_t* symbols,
                          int32_t* indexes, int32_t* classes, void* stream) {
  if (!x || !xhat || !dmap || !symbols || !indexes || !classes) return ICM_ERR_ARG;
  if (!side_ok(H) || !side_ok(W)) return ICM_ERR_ARG;
  const int gh = (H + CELL - 1) / CELL, gw = (W + CELL - 1) / CELL;
  const int strips = (gw + WAVES - 1) / WAVES;
  hipLaunchKernelGGL(residual_code_map_kernel, dim3((unsigned)(gh * strips)), dim3(BLOCK), 0, ST, x, xhat, H, W, dmap,
                     gw, strips, symbols, indexes, classes);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_residual_indexes(const int32_t* classes, int H, int W, int32_t* indexes, void* stream) {
  if (!side_ok(H) || !side_ok(W)) return ICM_ERR_ARG;
  return icm_residual_indexes_band(classes, H, W, 0, (int64_t)H * W, indexes, stream);
}

int icm_residual_indexes_band(const int32_t* classes, int H, int W, int64_t e_lo, int64_t e_hi, int32_t* indexes,
                              void* stream) {
  if (!classes || !indexes || !side_ok(H) || !side_ok(W) || !band_ok(H, W, e_lo, e_hi)) return ICM_ERR_ARG;
  const int rpr = (W + RUN - 1) / RUN;
  const int y_first = (int)(e_lo / W), y_last = (int)((e_hi - 1) / W);
  const long long total = (long long)(y_last - y_first + 1) * rpr;   // <= 32768 * 8192
  hipLaunchKernelGGL(residual_indexes_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ST, classes,
                     W, (W + CELL - 1) / CELL, Band{e_hi - e_lo, e_lo, e_hi}, y_first, indexes, rpr, total);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_residual_apply(const uint8_t* xhat, const int32_t* symbols, int H, int W, int y0, int x0, int h, int w, int D,
                       uint8_t* out, void* stream) {
  if (!side_ok(H) || !side_ok(W)) return ICM_ERR_ARG;
  return icm_residual_apply_band(xhat, symbols, H, W, 0, (int64_t)H * W, y0, x0, h, w, D, out, stream);
}

int icm_residual_apply_band(const uint8_t* xhat, const int32_t* symbols, int H, int W, int64_t e_lo, int64_t e_hi,
                            int y0, int x0, int h, int w, int D, uint8_t* out, void* stream) {
  if (!xhat || !symbols || !out) return ICM_ERR_ARG;
  if (!side_ok(H) || !side_ok(W) || !side_ok(h) || !side_ok(w) || D < 0 || D > MAX_D) return ICM_ERR_ARG;
  if (!band_ok(H, W, e_lo, e_hi) || !window_ok(H, W, y0, x0, h, w, e_lo, e_hi)) return ICM_ERR_ARG;
  const int rpr = (w + RUN - 1) / RUN;
  const long long total = (long long)h * rpr;
  hipLaunchKernelGGL(residual_apply_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ST, xhat,
                     symbols, Band{e_hi - e_lo, e_lo, e_hi}, W, y0, x0, h, w, 2 * D + 1, out, rpr, total);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

int icm_residual_apply_map(const uint8_t* xhat, const int32_t* symbols, int H, int W, int y0, int x0, int h, int w,
                           const uint8_t* dmap, uint8_t* out, void* stream) {
  if (!side_ok(H) || !side_ok(W)) return ICM_ERR_ARG;
  return icm_residual_apply_map_band(xhat, symbols, H, W, 0, (int64_t)H * W, y0, x0, h, w, dmap, out, stream);
}

int icm_residual_apply_map_band(const uint8_t* xhat, const int32_t* symbols, int H, int W, int64_t e_lo, int64_t e_hi,
                                int y0, int x0, int h, int w, const uint8_t* dmap, uint8_t* out, void* stream) {
  if (!xhat || !symbols || !dmap || !out) return ICM_ERR_ARG;
  if (!side_ok(H) || !side_ok(W) || !side_ok(h) || !side_ok(w)) return ICM_ERR_ARG;
  if (!band_ok(H, W, e_lo, e_hi) || !window_ok(H, W, y0, x0, h, w, e_lo, e_hi)) return ICM_ERR_ARG;
  const int rpr = (w + RUN - 1) / RUN;
  const long long total = (long long)h * rpr;
  hipLaunchKernelGGL(residual_apply_map_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ST, xhat,
                     symbols, Band{e_hi - e_lo, e_lo, e_hi}, W, y0, x0, h, w, dmap, (W + CELL - 1) / CELL, out, rpr,
                     total);
  ICM_CHECK_LAUNCH();
  return ICM_OK;
}

}  // extern "C"
