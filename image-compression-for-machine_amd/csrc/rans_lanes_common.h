// Lane streams (format in words: icm_amd/bitstream.py): the arithmetic of one lane's step, stated once for the host
// coder (csrc/rans.cpp, plain C++) and the kernels (csrc/rans_lanes.hip), and the parser of the header and length
// table.  Not here, because it is what differs: the order of the words inside a phase (a lane loop on the host, a ballot
// and a popcount of the lower lanes on the device) and the CDF search (std::upper_bound / cdf_search).
// Every function is in bounds for any argument that satisfies its stated precondition; none loops.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define ICM_LANES_FN __host__ __device__ __forceinline__
#else
#define ICM_LANES_FN inline
#endif

namespace icm {
namespace lanes {

constexpr int kLanes = 64;               // lanes (rANS states) per body
constexpr uint32_t kL = 1u << 16;        // lower bound of a state's interval; words are 16 bits
constexpr int kMaxG = 4096;              // bodies per stream
constexpr int kBodyMin = 4 * kLanes;     // bytes of a body without words: its 64 initial states

// The validity rule of a table, once, as text: a function in its place turns the kernels' branch round and hides
// stride >= 2 from the row offset (measured: 2 % slower binary-search decode on wide tables).  Size of table idx, 0 for an
// index outside the tables; a size fits if the table has a bin and lies inside its row, and only then may it be read.
#define ICM_LANES_SIZE(T, idx) (((idx) >= 0 && (idx) < (T).ncdf) ? (T).sizes[idx] : 0)
#define ICM_LANES_FITS(T, size) ((size) >= 2 && (size) <= (T).stride)

struct Tables {
  const int32_t* cdfs;
  const int32_t* sizes;
  const int32_t* offsets;
  int stride, ncdf;
  ICM_LANES_FN bool ok() const { return cdfs && sizes && offsets && ncdf > 0 && stride >= 2; }
  ICM_LANES_FN bool ok(int idx) const { return ICM_LANES_FITS(*this, ICM_LANES_SIZE(*this, idx)); }
};

// elements of a run of n that one body codes (body g: [g c, min(n, (g + 1) c))
ICM_LANES_FN int64_t chunk(int64_t n, int G) { return ((n + G - 1) / G + kLanes - 1) / kLanes * kLanes; }

// the puts of one element: phase 0 is the table symbol, phases 1..3 the raw 16-bit groups of a lane that escaped
struct Puts {
  uint32_t start0, freq0;
  uint64_t raw;                          // zig-zag of the escape value: odd below the table, even above; 48 bits coded
  bool esc;
  ICM_LANES_FN bool has(int ph) const { return ph == 0 || esc; }
  ICM_LANES_FN uint32_t freq(int ph) const { return ph == 0 ? freq0 : 1u; }
  ICM_LANES_FN uint32_t start(int ph) const { return ph == 0 ? start0 : (uint32_t)((raw >> (16 * (ph - 1))) & 0xFFFF); }
};

// symbol -> puts; size = ICM_LANES_SIZE(T, idx) fits.  false: the bin has no width, or a width no 16-bit put can code
ICM_LANES_FN bool plan(const Tables& T, int idx, int size, int32_t symbol, Puts& p) {
  const int32_t* cdf = T.cdfs + (int64_t)idx * T.stride;
  const int overflow = size - 2;                         // index of the escape bin
  int64_t v = (int64_t)symbol - T.offsets[idx];
  p.raw = 0, p.esc = false;
  if (v < 0) { p.raw = (uint64_t)(-2 * v - 1); v = overflow; p.esc = true; }
  else if (v >= overflow) { p.raw = (uint64_t)(2 * (v - overflow)); v = overflow; p.esc = true; }
  const int lo = cdf[v], hi = cdf[v + 1];
  p.start0 = (uint32_t)lo, p.freq0 = (uint32_t)(hi - lo);
  return hi > lo && lo >= 0 && hi <= 65536 && hi - lo <= 0xFFFF;
}

// the put of (start, freq) out of 2^16: if put_emits, x & 0xFFFF leaves as a word and x >>= 16 first
ICM_LANES_FN bool put_emits(uint32_t x, uint32_t freq) { return x >= (freq << 16); }   // freq <= 0xFFFF: no overflow
ICM_LANES_FN uint32_t put(uint32_t x, uint32_t start, uint32_t freq) { return ((x / freq) << 16) + x % freq + start; }

// the decoder's advance over the bin [lo, hi) that the search found for cum = x & 0xFFFF, if cum is in it
ICM_LANES_FN bool in_bin(int cum, int lo, int hi) { return lo <= cum && cum < hi; }
ICM_LANES_FN uint32_t advance(uint32_t x, int cum, int lo, int hi) {
  return (uint32_t)(hi - lo) * (x >> 16) + (uint32_t)(cum - lo);
}

// symbol of an escape from its raw groups, in 64 bits: one that is not is_int32 is ICM_LANES_ST_ESCAPE
ICM_LANES_FN long long unescape(unsigned long long raw, int overflow, int offset) {
  const long long half = (long long)(raw >> 1);
  return ((raw & 1) ? -half - 1 : half + overflow) + offset;
}
ICM_LANES_FN bool is_int32(long long v) { return v >= INT32_MIN && v <= INT32_MAX; }

// ---- header and length table (host side of either decoder)
inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

struct Body {
  int64_t off;      // byte offset of the body in the string: its 64 states, then its words
  int64_t words;    // u16 words after the states
};

// "ICML", version 1, G, G lengths that tile the rest of the string exactly -> bodies[G]; false: not a lane stream
inline bool parse(const uint8_t* s, int64_t n, std::vector<Body>& bodies) {
  if (!s || n < 8 || std::memcmp(s, "ICML", 4) != 0) return false;
  const int64_t G = le16(s + 6);
  if (le16(s + 4) != 1 || G < 1 || G > kMaxG || 8 + 4 * G > n) return false;
  int64_t pos = 8 + 4 * G;
  for (int64_t g = 0; g < G; ++g) {
    const int64_t len = le32(s + 8 + 4 * g);
    if (len < kBodyMin || (len & 1) || pos + len > n) return false;
    bodies.push_back({pos, (len - kBodyMin) / 2});
    pos += len;
  }
  return pos == n;
}

}  // namespace lanes
}  // namespace icm
