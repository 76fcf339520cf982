// Entropy-coding back end of update() / compress() / decompress(): quantised CDF tables and the interleaved
// 64-bit rANS stream.  HOST code (the reference codes on the host too: compressai/entropy_models/
// entropy_models.py:172-290 hands Python lists to the `compressai.ans` / `compressai._CXX` extensions).
//
// What this replaces.  The reference tree ships those two extensions only as cp38 binaries (never loaded here); their
// sources (CompressAI 1.1.6dev0, compressai/cpp_exts/{rans,ops}) are absent from /root/reference.  The arithmetic
// core they wrap IS in the tree: third_party/ryg_rans/rans64.h (public domain, F. Giesen).  This file restates
//   * the rans64.h state machine (Rans64EncPut / EncFlush / DecInit / DecGet / DecAdvance; rans64.h:62-142) --
//     pinned bit for bit against that very header by tests/test_rans_codec.py (oracle/_ref builds a shim from it);
//   * CompressAI's published interface conventions on top of it: 16-bit precision, symbols shifted by the table's
//     offset, values outside the table escaped through the last ("overflow") bin and written as 4-bit bypass groups
//     (count in unary-ish nibbles, then the zig-zagged magnitude), one stream per call, symbols pushed in reverse;
//   * pmf_to_quantized_cdf: round(p * 2^precision), renormalise to 2^precision, cumulate, then steal counts from the
//     least frequent symbol with more than one count until no symbol has zero width.
// Parity status: round-trip identity and the rans64.h pin are tested; equality with the reference's own byte
// streams is "parity unpinned"  because the reference's coder binaries may not be run.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/icm_hip.h"
#include "rans_lanes_common.h"

namespace {

constexpr uint32_t kPrecision = 16;        // entropy_coder_precision (entropy_models.py:78-81)
constexpr uint32_t kBypassBits = 4;        // escape payload granularity
constexpr uint32_t kBypassMax = (1u << kBypassBits) - 1;
constexpr uint64_t kRansL = 1ull << 31;    // lower bound of the normalisation interval (rans64.h:58)

// ---- rANS state machine (word-wise renormalisation, 63-bit state) -----------------------------------------------
struct Enc {
  uint64_t x = kRansL;                     // Rans64EncInit
  std::vector<uint32_t> words;             // emitted renormalisation words, in emission order (stream is reversed)
  // x = C(s, x) for a symbol with cumulative start `start`, width `freq`, out of 2^bits   (rans64.h:73-90)
  inline void put(uint32_t start, uint32_t freq, uint32_t bits) {
    const uint64_t x_max = ((kRansL >> bits) << 32) * freq;
    if (x >= x_max) {
      words.push_back((uint32_t)x);
      x >>= 32;
    }
    x = ((x / freq) << bits) + (x % freq) + start;
  }
  // raw bits: a symbol of width 1 out of 2^nbits whose start is the value (uniform distribution)
  inline void put_bits(uint32_t val, uint32_t nbits) {
    const uint32_t freq = 1u << (kPrecision - nbits);
    const uint64_t x_max = ((kRansL >> kPrecision) << 32) * freq;
    if (x >= x_max) {
      words.push_back((uint32_t)x);
      x >>= 32;
    }
    x = (x << nbits) | val;
  }
};

struct Dec {
  const uint32_t* p = nullptr;
  const uint32_t* end = nullptr;
  uint64_t x = 0;
  bool bad = false;
  inline uint32_t next() {
    if (p >= end) { bad = true; return 0; }
    return *p++;
  }
  void init(const uint32_t* s, const uint32_t* e) {   // Rans64DecInit (rans64.h:102-110)
    p = s; end = e; bad = false;
    const uint64_t lo = next(), hi = next();
    x = lo | (hi << 32);
  }
  inline uint32_t peek(uint32_t bits) const { return (uint32_t)(x & ((1u << bits) - 1)); }   // Rans64DecGet
  inline void advance(uint32_t start, uint32_t freq, uint32_t bits) {                           // Rans64DecAdvance
    const uint64_t mask = (1ull << bits) - 1;
    x = freq * (x >> bits) + (x & mask) - start;
    if (x < kRansL) x = (x << 32) | next();
  }
  inline uint32_t get_bits(uint32_t nbits) {
    const uint32_t v = (uint32_t)(x & ((1u << nbits) - 1));
    x >>= nbits;
    if (x < kRansL) x = (x << 32) | next();
    return v;
  }
};

using icm::lanes::Tables;     // one table struct and validity rule for both streams (rans_lanes_common.h)

struct Item {
  uint16_t start, width;
  bool raw;
};

// symbols -> (start, width) items in FORWARD order; the stream is then produced by pushing them in reverse
int plan_items(const int32_t* symbols, const int32_t* indexes, int64_t n, const Tables& T, std::vector<Item>& items) {
  items.reserve(items.size() + (size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int idx = indexes[i];
    if (!T.ok(idx)) return ICM_ERR_ARG;
    const int32_t* cdf = T.cdfs + (int64_t)idx * T.stride;
    const int32_t overflow = T.sizes[idx] - 2;       // index of the escape bin
    int64_t v = (int64_t)symbols[i] - T.offsets[idx];
    uint64_t raw = 0;                                // 64-bit: |symbol| up to 2^31 needs 33 bits after the zig-zag
    if (v < 0) {
      raw = (uint64_t)(-2 * v - 1);                  // odd  = below the table
      v = overflow;
    } else if (v >= overflow) {
      raw = (uint64_t)(2 * (v - overflow));          // even = above the table (0 = exactly the last regular bin + 1)
      v = overflow;
    }
    const int32_t lo = cdf[v], hi = cdf[v + 1];
    if (hi <= lo || lo < 0 || hi > (1 << kPrecision)) return ICM_ERR_ARG;   // zero-width symbol: table not usable
    items.push_back({(uint16_t)lo, (uint16_t)(hi - lo), false});
    if (v == overflow) {
      uint32_t groups = 0;
      while ((raw >> (groups * kBypassBits)) != 0) ++groups;
      uint32_t c = groups;
      while (c >= kBypassMax) {                      // group count: nibbles of 15 until the remainder is < 15
        items.push_back({(uint16_t)kBypassMax, 1, true});
        c -= kBypassMax;
      }
      items.push_back({(uint16_t)c, 1, true});
      for (uint32_t j = 0; j < groups; ++j)
        items.push_back({(uint16_t)((raw >> (j * kBypassBits)) & kBypassMax), 1, true});
    }
  }
  return ICM_OK;
}

int64_t emit(const std::vector<Item>& items, uint8_t* out, int64_t cap) {
  Enc e;
  e.words.reserve(items.size() / 2 + 4);
  for (size_t k = items.size(); k-- > 0;) {
    const Item& it = items[k];
    if (it.raw) e.put_bits(it.start, kBypassBits);
    else e.put(it.start, it.width, kPrecision);
  }
  // Rans64EncFlush (rans64.h:93-100): the final state heads the stream, low word first; the renormalisation words
  // follow in reverse emission order (the encoder writes backwards, the decoder reads forwards)
  const int64_t nwords = (int64_t)e.words.size() + 2;
  if (out) {
    if (cap < nwords * 4) return -1;
    uint32_t* w = reinterpret_cast<uint32_t*>(out);
    uint32_t tmp;
    tmp = (uint32_t)e.x; std::memcpy(w, &tmp, 4);
    tmp = (uint32_t)(e.x >> 32); std::memcpy(w + 1, &tmp, 4);
    for (int64_t k = 0; k < (int64_t)e.words.size(); ++k)
      std::memcpy(w + 2 + k, &e.words[e.words.size() - 1 - k], 4);
  }
  return nwords * 4;
}

int decode_run(Dec& d, const int32_t* indexes, int64_t n, const Tables& T, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) {
    const int idx = indexes[i];
    if (!T.ok(idx)) return ICM_ERR_ARG;
    const int32_t* cdf = T.cdfs + (int64_t)idx * T.stride;
    const int32_t size = T.sizes[idx], overflow = size - 2;
    const uint32_t cum = d.peek(kPrecision);
    // first table entry above the cumulative value (tables are short: binary search over [0, size))
    const int32_t* it = std::upper_bound(cdf, cdf + size, (int32_t)cum);
    int32_t s = (int32_t)(it - cdf) - 1;
    if (s < 0 || s > overflow) return ICM_ERR_ARG;
    d.advance((uint32_t)cdf[s], (uint32_t)(cdf[s + 1] - cdf[s]), kPrecision);
    int32_t v = s;
    if (s == overflow) {
      uint32_t c = d.get_bits(kBypassBits), groups = c;
      while (c == kBypassMax) {
        c = d.get_bits(kBypassBits);
        groups += c;
        if (groups > 16 || d.bad) return ICM_ERR_ARG;   // 16 nibbles = 64 payload bits
      }
      if (groups > 16) return ICM_ERR_ARG;
      uint64_t raw = 0;
      for (uint32_t j = 0; j < groups; ++j) raw |= (uint64_t)d.get_bits(kBypassBits) << (j * kBypassBits);
      const int64_t half = (int64_t)(raw >> 1);
      const int64_t vv = (raw & 1) ? -half - 1 : half + overflow;
      if (vv < INT32_MIN || vv > INT32_MAX) return ICM_ERR_ARG;
      v = (int32_t)vv;
    }
    if (d.bad) return ICM_ERR_ARG;                   // ran past the end of the stream: truncated / corrupt input
    out[i] = v + T.offsets[idx];
  }
  return ICM_OK;
}

struct Decoder {
  std::vector<uint32_t> words;
  Dec d;
};

// ---- lane streams: 64 interleaved 32-bit rANS states per wave body (format: icm_amd/bitstream.py) ----------------
// The executable definition the kernels of rans_lanes.hip are held to: the arithmetic of a lane's step is
// rans_lanes_common.h, which the kernels compile too; the loops below add the order.  One body = 64 initial decoder
// states, then the 16-bit words in the order the decoder reads them; a step of 64 elements runs four phases (table
// symbol, then three raw 16-bit groups for the lanes that escaped), and inside a phase the lanes that renormalise take
// consecutive words in ascending lane order.  Every loop is counted by the run lengths and G, never by stream contents.
using namespace icm::lanes;

struct LaneDecoder {
  std::vector<uint8_t> data;
  int G = 0;
  std::vector<Body> body;
  std::vector<uint32_t> x;                     // [G][64]
  std::vector<int64_t> cur;                    // [G] word cursor
  std::vector<int> status;                     // [G] ICM_LANES_ST_* bits of each wave, sticky
  inline uint32_t word(int g, int64_t k) {
    if (k >= body[g].words) { status[g] |= ICM_LANES_ST_OVERRUN; return 0; }
    return le16(data.data() + body[g].off + kBodyMin + 2 * k);
  }
  inline int status_of(int g0, int g1) const {
    int st = 0;
    for (int g = g0; g < g1; ++g) st |= status[g];
    return st;
  }
};

// waves g0 <= g < g1 decode their elements of a run of n (the whole run's length: it fixes c); element e reads
// indexes[e - elem0] and writes out[e - elem0].  The whole run is (0, G, 0).  No other wave is touched.
void lanes_decode_run(LaneDecoder& D, int g0, int g1, int64_t elem0, const int32_t* indexes, int64_t n, const Tables& T,
                      int32_t* out) {
  const int64_t c = chunk(n, D.G);
  for (int g = g0; g < g1; ++g) {
    int& status = D.status[g];
    uint32_t* x = D.x.data() + (size_t)g * kLanes;
    const int64_t e0 = (int64_t)g * c, e1 = std::min(n, e0 + c);
    for (int64_t base = e0; base < e1; base += kLanes) {
      const int act = (int)std::min<int64_t>(kLanes, e1 - base);
      bool esc[kLanes];
      uint64_t raw[kLanes];
      int32_t overflow[kLanes];
      int64_t k = D.cur[g];
      const int32_t* ix = indexes + (base - elem0);   // base >= g0 c >= elem0
      int32_t* o = out + (base - elem0);
      for (int l = 0; l < act; ++l) {              // phase 0: the table symbol
        esc[l] = false;
        raw[l] = 0;
        o[l] = 0;
        const int idx = ix[l], size = ICM_LANES_SIZE(T, idx);
        if (!ICM_LANES_FITS(T, size)) { status |= ICM_LANES_ST_INDEX; overflow[l] = -1; continue; }
        const int32_t* cdf = T.cdfs + (int64_t)idx * T.stride;
        overflow[l] = size - 2;
        const int cum = (int)(x[l] & 0xFFFF);
        const int32_t s = (int32_t)(std::upper_bound(cdf, cdf + size, (int32_t)cum) - cdf) - 1;
        if (s < 0 || s > overflow[l] || cdf[s + 1] <= cdf[s]) { status |= ICM_LANES_ST_SYMBOL; overflow[l] = -1; continue; }
        x[l] = advance(x[l], cum, cdf[s], cdf[s + 1]);
        if (x[l] < kL) x[l] = (x[l] << 16) | D.word(g, k++);
        esc[l] = s == overflow[l];
        o[l] = s + T.offsets[idx];
      }
      for (int ph = 0; ph < 3; ++ph)               // phases 1..3: raw 16-bit groups of the lanes that escaped
        for (int l = 0; l < act; ++l)
          if (esc[l]) {
            raw[l] |= (uint64_t)(x[l] & 0xFFFF) << (16 * ph);
            x[l] = (x[l] & 0xFFFF0000u) | D.word(g, k++);
          }
      for (int l = 0; l < act; ++l)
        if (esc[l]) {
          const int64_t v = unescape(raw[l], overflow[l], T.offsets[ix[l]]);
          if (is_int32(v)) o[l] = (int32_t)v;
          else { status |= ICM_LANES_ST_ESCAPE; o[l] = 0; }
        }
      D.cur[g] = k;
    }
  }
}

}  // namespace

extern "C" {

int icm_rans_lanes_waves(const int64_t* run_lengths, int nruns, int64_t symbols_per_wave) {
  if (nruns < 0 || (nruns > 0 && !run_lengths) || symbols_per_wave < 1) return -1;
  int64_t nmax = 0;
  for (int r = 0; r < nruns; ++r) {
    if (run_lengths[r] < 0) return -1;
    nmax = std::max(nmax, run_lengths[r]);
  }
  const int64_t g = (nmax + symbols_per_wave - 1) / symbols_per_wave;
  return (int)std::min<int64_t>(std::max<int64_t>(g, 1), kMaxG);
}

int64_t icm_rans_lanes_encode(const int32_t* symbols, const int32_t* indexes, const int64_t* run_lengths, int nruns,
                              const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                              int ncdf, int64_t symbols_per_wave, uint8_t* out, int64_t out_capacity) {
  const Tables T{cdfs, cdf_sizes, offsets, cdf_stride, ncdf};
  const int G = icm_rans_lanes_waves(run_lengths, nruns, symbols_per_wave);
  if (G < 1 || !T.ok()) return -1;
  int64_t total = 0;
  for (int r = 0; r < nruns; ++r) total += run_lengths[r];
  if (total > 0 && (!symbols || !indexes)) return -1;
  try {
    std::vector<int64_t> run_off((size_t)nruns + 1, 0);
    for (int r = 0; r < nruns; ++r) run_off[r + 1] = run_off[r] + run_lengths[r];
    std::vector<std::vector<uint16_t>> words((size_t)G);   // per body, in emission order (the body holds them reversed)
    std::vector<uint32_t> states((size_t)G * kLanes, kL);
    for (int g = 0; g < G; ++g) {
      uint32_t* x = states.data() + (size_t)g * kLanes;
      std::vector<uint16_t>& w = words[g];
      for (int r = nruns - 1; r >= 0; --r) {
        const int64_t n = run_lengths[r], c = chunk(n, G);
        const int64_t e0 = (int64_t)g * c, e1 = std::min(n, e0 + c);
        if (e1 <= e0) continue;
        const int64_t steps = (e1 - e0 + kLanes - 1) / kLanes;
        for (int64_t t = steps - 1; t >= 0; --t) {
          const int64_t base = e0 + t * kLanes;
          const int act = (int)std::min<int64_t>(kLanes, e1 - base);
          Puts it[kLanes];
          for (int l = 0; l < act; ++l) {
            const int64_t e = run_off[r] + base + l;
            const int idx = indexes[e], size = ICM_LANES_SIZE(T, idx);
            if (!ICM_LANES_FITS(T, size) || !plan(T, idx, size, symbols[e], it[l])) return -1;
          }
          for (int ph = 3; ph >= 0; --ph)
            for (int l = act - 1; l >= 0; --l) {     // descending lanes going down = ascending lanes in the body
              if (!it[l].has(ph)) continue;
              const uint32_t freq = it[l].freq(ph);
              if (put_emits(x[l], freq)) { w.push_back((uint16_t)(x[l] & 0xFFFF)); x[l] >>= 16; }
              x[l] = put(x[l], it[l].start(ph), freq);
            }
        }
      }
    }
    int64_t nbytes = 8 + 4 * (int64_t)G;
    for (int g = 0; g < G; ++g) nbytes += kBodyMin + 2 * (int64_t)words[g].size();
    if (!out) return nbytes;
    if (out_capacity < nbytes) return -1;
    auto put16 = [](uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); };
    auto put32 = [](uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); };
    std::memcpy(out, "ICML", 4);
    put16(out + 4, 1);
    put16(out + 6, (uint32_t)G);
    uint8_t* p = out + 8 + 4 * (int64_t)G;
    for (int g = 0; g < G; ++g) {
      const std::vector<uint16_t>& w = words[g];
      put32(out + 8 + 4 * g, (uint32_t)(kBodyMin + 2 * w.size()));
      for (int l = 0; l < kLanes; ++l, p += 4) put32(p, states[(size_t)g * kLanes + l]);
      for (size_t k = w.size(); k-- > 0; p += 2) put16(p, w[k]);
    }
    return nbytes;
  } catch (const std::bad_alloc&) {
    return -1;
  }
}

void* icm_rans_lanes_decoder_create(const uint8_t* stream, int64_t nbytes) {
  if (!stream || nbytes < 8) return nullptr;
  LaneDecoder* D = new (std::nothrow) LaneDecoder();
  if (!D) return nullptr;
  try {
    D->data.assign(stream, stream + nbytes);
    if (parse(D->data.data(), nbytes, D->body)) {
      D->G = (int)D->body.size();
      D->cur.assign((size_t)D->G, 0);
      D->status.assign((size_t)D->G, 0);
      D->x.resize((size_t)D->G * kLanes);
      for (int g = 0; g < D->G; ++g)
        for (int l = 0; l < kLanes; ++l) D->x[(size_t)g * kLanes + l] = le32(D->data.data() + D->body[g].off + 4 * l);
      return D;
    }
  } catch (const std::bad_alloc&) {
  }
  delete D;
  return nullptr;
}

int icm_rans_lanes_decoder_decode_run(void* handle, const int32_t* indexes, int64_t n, const int32_t* cdfs,
                                      int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int ncdf,
                                      int32_t* out) {
  const Tables T{cdfs, cdf_sizes, offsets, cdf_stride, ncdf};
  if (!handle || n < 0 || (n > 0 && (!indexes || !out)) || !T.ok()) return ICM_ERR_ARG;
  LaneDecoder& D = *static_cast<LaneDecoder*>(handle);
  return icm_rans_lanes_decoder_decode_run_waves(handle, 0, D.G, 0, indexes, n, cdfs, cdf_stride, cdf_sizes, offsets, ncdf,
                                                 out);
}

int icm_rans_lanes_decoder_decode_run_waves(void* handle, int g0, int g1, int64_t elem0, const int32_t* indexes,
                                            int64_t n, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                                            const int32_t* offsets, int ncdf, int32_t* out) {
  const Tables T{cdfs, cdf_sizes, offsets, cdf_stride, ncdf};
  if (!handle || n < 0 || !T.ok()) return ICM_ERR_ARG;
  LaneDecoder& D = *static_cast<LaneDecoder*>(handle);
  const int64_t c = chunk(n, D.G);
  if (g0 < 0 || g0 > g1 || g1 > D.G || elem0 < 0 || elem0 > (int64_t)g0 * c) return ICM_ERR_ARG;
  const bool owns = g0 < g1 && (int64_t)g0 * c < n;   // a range that owns no element needs no buffers
  if (owns && (!indexes || !out)) return ICM_ERR_ARG;
  if (owns) lanes_decode_run(D, g0, g1, elem0, indexes, n, T, out);
  return D.status_of(g0, g1) ? ICM_ERR_ARG : ICM_OK;
}

int icm_rans_lanes_decoder_finish(void* handle) {
  if (!handle) return -1;
  return icm_rans_lanes_decoder_finish_waves(handle, 0, static_cast<LaneDecoder*>(handle)->G, 1);
}

int icm_rans_lanes_decoder_finish_waves(void* handle, int g0, int g1, int end) {
  if (!handle) return -1;
  LaneDecoder& D = *static_cast<LaneDecoder*>(handle);
  if (g0 < 0 || g0 > g1 || g1 > D.G) return -1;
  for (int g = g0; end && g < g1; ++g) {
    if (D.cur[g] != D.body[g].words) D.status[g] |= ICM_LANES_ST_CURSOR;
    for (int l = 0; l < kLanes; ++l)
      if (D.x[(size_t)g * kLanes + l] != kL) D.status[g] |= ICM_LANES_ST_STATE;
  }
  return D.status_of(g0, g1);
}

int icm_rans_lanes_decoder_waves(void* handle) { return handle ? static_cast<LaneDecoder*>(handle)->G : -1; }

void icm_rans_lanes_decoder_destroy(void* handle) { delete static_cast<LaneDecoder*>(handle); }

int icm_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf) {
  if (!pmf || !cdf || n < 1 || precision < 1 || precision > 16) return ICM_ERR_ARG;
  for (int i = 0; i < n; ++i)
    if (!(pmf[i] >= 0.0f) || !std::isfinite(pmf[i])) return ICM_ERR_ARG;   // domain error in the reference
  const uint32_t one = 1u << precision;
  std::vector<uint32_t> c((size_t)n + 1);
  c[0] = 0;
  uint64_t total = 0;
  for (int i = 0; i < n; ++i) {
    c[i + 1] = (uint32_t)std::round(pmf[i] * (float)one);
    total += c[i + 1];
  }
  if (total == 0) return ICM_ERR_ARG;
  uint32_t run = 0;
  for (int i = 0; i <= n; ++i) {                     // renormalise each count to the 2^precision budget, cumulate
    run += (uint32_t)(((uint64_t)one * c[i]) / total);
    c[i] = run;
  }
  c[n] = one;
  for (int i = 0; i < n; ++i) {
    if (c[i] != c[i + 1]) continue;
    // symbol i has zero width: take one count from the narrowest symbol that can spare one
    uint32_t best = ~0u;
    int donor = -1;
    for (int j = 0; j < n; ++j) {
      const uint32_t f = c[j + 1] - c[j];
      if (f > 1 && f < best) { best = f; donor = j; }
    }
    if (donor < 0) return ICM_ERR_ARG;               // more symbols than counts
    if (donor < i) for (int j = donor + 1; j <= i; ++j) --c[j];
    else for (int j = i + 1; j <= donor; ++j) ++c[j];
  }
  for (int i = 0; i <= n; ++i) cdf[i] = (int32_t)c[i];
  return ICM_OK;
}

int64_t icm_rans_encode_with_indexes(const int32_t* symbols, const int32_t* indexes, int64_t n, const int32_t* cdfs,
                                     int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int ncdf,
                                     uint8_t* out, int64_t out_capacity) {
  const Tables T{cdfs, cdf_sizes, offsets, cdf_stride, ncdf};
  if (n < 0 || (n > 0 && (!symbols || !indexes)) || !T.ok()) return -1;
  std::vector<Item> items;
  try {
    if (plan_items(symbols, indexes, n, T, items) != ICM_OK) return -1;
    return emit(items, out, out_capacity);
  } catch (const std::bad_alloc&) {
    return -1;
  }
}

int icm_rans_decode_with_indexes(const uint8_t* stream, int64_t nbytes, const int32_t* indexes, int64_t n,
                                 const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                                 int ncdf, int32_t* out) {
  void* h = icm_rans_decoder_create(stream, nbytes);
  if (!h) return ICM_ERR_ARG;
  const int rc = icm_rans_decoder_decode(h, indexes, n, cdfs, cdf_stride, cdf_sizes, offsets, ncdf, out);
  icm_rans_decoder_destroy(h);
  return rc;
}

void* icm_rans_decoder_create(const uint8_t* stream, int64_t nbytes) {
  if (!stream || nbytes < 8 || (nbytes & 3)) return nullptr;
  Decoder* D = new (std::nothrow) Decoder();
  if (!D) return nullptr;
  try {
    D->words.resize((size_t)(nbytes / 4));
  } catch (const std::bad_alloc&) {
    delete D;
    return nullptr;
  }
  std::memcpy(D->words.data(), stream, (size_t)nbytes);
  D->d.init(D->words.data(), D->words.data() + D->words.size());
  return D;
}

int icm_rans_decoder_decode(void* handle, const int32_t* indexes, int64_t n, const int32_t* cdfs, int cdf_stride,
                            const int32_t* cdf_sizes, const int32_t* offsets, int ncdf, int32_t* out) {
  const Tables T{cdfs, cdf_sizes, offsets, cdf_stride, ncdf};
  if (!handle || n < 0 || (n > 0 && (!indexes || !out)) || !T.ok()) return ICM_ERR_ARG;
  return decode_run(static_cast<Decoder*>(handle)->d, indexes, n, T, out);
}

void icm_rans_decoder_destroy(void* handle) { delete static_cast<Decoder*>(handle); }

}  // extern "C"
