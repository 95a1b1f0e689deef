// Host side of the C ABI (include/meyda_gpu.h): plan construction, host tables,
// device residency, launches and error reporting.
//
// Host tables follow the reference formulas evaluated in IEEE double exactly as
// the JavaScript does (this file is compiled with -ffp-contract=off); the
// golden tests compare them bit-for-bit with the reference's own tables
// (tests/test_capi_host.py).
#include <hip/hip_runtime.h>
#include <emmintrin.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "mgx_internal.h"

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace mgx {
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  const int code = (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) ? MGX_E_OUT_OF_MEMORY : MGX_E_DEVICE;
  return fail(code, "%s: %s", what, hipGetErrorString(e));
}
}  // namespace mgx

namespace {
using mgx::fail;
using mgx::hip_fail;

const uint64_t kHostChunk = 65536;              // frames per host-staging chunk (up to N = 2048: host_chunk)
// A staging slot never exceeds the bytes it has at N = 2048 (512 MiB, two of them): above it a chunk holds
// as many frames fewer, 32,768 at N = 4096 (host_chunk below).
const uint64_t kHostSlotFloats = kHostChunk * 2048;
// Host batches of at most this many frames (a real-time buffer, or a streaming batch of K
// buffers) skip the device staging: the frames are copied into plan-owned pinned host memory
// that the kernel reads over PCIe itself, and it writes the features back there (no DMA copies,
// no cross-stream events: one launch and one stream synchronisation per call). Overridden by
// $MGX_SMALL_BATCH_FRAMES at plan creation (0: always the staged path).
const uint64_t kSmallBatchFrames = 512;
// How long the small path spins on its completion word before it blocks on the stream (a
// 512-frame batch takes ~0.1 ms; a longer wait is a busy device, where blocking frees the core).
const int kSmallSpinUs = 2000;
// Resident launches (MGX_FLAG_RESIDENT) started and not yet seen to end, per device: each holds one workgroup
// slot of one CU, so the persistent grid of any other launch on the device is that much smaller (a grid of
// exactly the resident workgroups would leave one workgroup -- its whole share of the launch -- waiting for a
// slot until the others finish: twice the launch time).
constexpr int kMaxDevices = 64;
std::atomic<int> g_resident_live[kMaxDevices];
const double kJsPi = 3.141592653589793;        // Math.PI
const double kJsSqrt1_2 = 0.7071067811865476;  // Math.SQRT1_2

const char* const kNames[MGX_NUM_FEATURES] = {
    "rms", "energy", "zcr", "spectralCentroid", "spectralFlatness", "spectralSlope",
    "spectralRolloff", "spectralSpread", "spectralSkewness", "spectralKurtosis",
    "loudness.total", "perceptualSpread", "perceptualSharpness", "loudness", "mfcc",
    "amplitudeSpectrum", "powerSpectrum", "complexSpectrum", "buffer", "melBands"};

// src/feature-info.js:1-65
const int kInfo[MGX_NUM_FEATURES] = {
    MGX_TYPE_NUMBER, MGX_TYPE_NUMBER, MGX_TYPE_NUMBER, MGX_TYPE_NUMBER, MGX_TYPE_NUMBER,
    MGX_TYPE_NUMBER, MGX_TYPE_NUMBER, MGX_TYPE_NUMBER, MGX_TYPE_NUMBER, MGX_TYPE_NUMBER,
    MGX_TYPE_NUMBER, MGX_TYPE_NUMBER, MGX_TYPE_NUMBER, MGX_TYPE_MULTIPLE_ARRAYS, MGX_TYPE_ARRAY,
    MGX_TYPE_ARRAY, MGX_TYPE_ARRAY, MGX_TYPE_MULTIPLE_ARRAYS, MGX_TYPE_ARRAY, MGX_TYPE_ARRAY};

// --------------------------------------------------------------- host tables
// src/meyda.js:128-138
void hanning(int n, float* out) {
  for (int i = 0; i < n; i++) out[i] = (float)(0.5 - 0.5 * cos(2 * kJsPi * i / (n - 1)));
}
// src/meyda.js:116-126
void hamming(int n, float* out) {
  for (int i = 0; i < n; i++) out[i] = (float)(0.54 - 0.46 * cos(2 * kJsPi * ((double)i / n - 1)));
}
// src/meyda.js:170-182 (the frequency is stored to a Float32Array, then read back)
void bark_scale(int n, double sr, float* out) {
  for (int i = 0; i < n; i++) {
    const float f = (float)((double)i * sr / n);
    const double q = (double)f / 7518;
    out[i] = (float)(13 * atan((double)f / 1315.8) + 3.5 * atan(q * q));
  }
}
// src/extractors/loudness.js:24-45. len = N/2 is 0 for bufferSize 1 (a power of two the
// reference accepts): barkScale[-1] is undefined there, so bandEnd is NaN, no limit moves
// and the last one is length - 1 = -1.
void bark_limits(const float* bark, int len, int nb, int32_t* lim) {
  if (len <= 0) {
    for (int i = 0; i < nb; i++) lim[i] = 0;
    lim[nb] = len - 1;
    return;
  }
  double end = (double)bark[len - 1] / nb;
  int band = 1;
  for (int i = 0; i <= nb; i++) lim[i] = 0;
  for (int i = 0; i < len; i++) {
    while ((double)bark[i] > end) {
      if (band <= nb) lim[band] = i;
      band++;
      end = (double)band * bark[len - 1] / nb;
    }
  }
  lim[nb] = len - 1;
}
// src/extractors/mfcc.js:7-38
void mel_bins(int n, double sr, int nf, int32_t* bins) {
  const double lo = 1125 * log(1 + (0.0 / 700));
  const double hi = 1125 * log(1 + ((sr / 2) / 700));
  const double step = (hi - lo) / (nf + 1);
  for (int i = 0; i < nf + 2; i++) {
    const float mv = (float)(i * step);
    const float mf = (float)(700 * (exp((double)mv / 1125) - 1));
    bins[i] = (int32_t)floor((double)(n + 1) * mf / sr);
  }
}
// src/extractors/mfcc.js:67-83
void dct_table(int nf, int nc, float* dct) {
  const double k = kJsPi / nf, w1 = 1.0 / sqrt((double)nf), w2 = sqrt(2.0 / nf);
  for (int i = 0; i < nc; i++)
    for (int j = 0; j < nf; j++) dct[i + j * nc] = (float)((i == 0 ? w1 : w2) * cos(k * (i + 1) * (j + 0.5)));
}
// Logical Hermitian index stored at each slot location of a size-m block.
void klist(int m, std::vector<int>& k) {
  k.assign(m / 2, 0);
  if (m == 2) return;
  std::vector<int> sub;
  klist(m / 2, sub);
  const int w = m / 2, h = w / 2;
  k[0] = 0;
  k[h] = w / 2;
  for (int a = 1; a < h; a++) {
    k[a] = sub[a];
    k[h + a] = w - sub[a];
  }
}
// lib/jsfft/fft.js:140-165: per stage, f_j by the recurrence from (cos pi/w, sin pi/w).
// Entry a of stage q (input blocks of w = 2^(q+1) samples, offset 2^q - 1) holds
// SQRT1_2 * f_{k(a)} (a = 0: SQRT1_2 * f_0); entry N/2 - 1 + q holds SQRT1_2 * f_{w/2}
// (the block-start pair, kernels.hip bfly_special / bfly_mixed).
void twiddles(int n, std::vector<double>& tw) {
  const int L = n / 2;
  int stages = 0;
  for (int w = 2; w <= L; w <<= 1) ++stages;
  tw.assign(2 * (size_t)(L - 1 + stages), 0.0);
  size_t off = 0;
  for (int w = 2; w <= L; w <<= 1) {
    const int h = w / 2;
    const double dr = cos(kJsPi / w), di = sin(kJsPi / w);
    std::vector<double> fr(w), fi(w);
    double r = 1, i = 0;
    for (int j = 0; j < w; j++) {
      fr[j] = r;
      fi[j] = i;
      const double t = r * dr - i * di;
      i = r * di + i * dr;
      r = t;
    }
    std::vector<int> kl;
    klist(w, kl);
    for (int a = 0; a < h; a++) {
      const int k = a == 0 ? 0 : kl[a];
      tw[2 * (off + a)] = kJsSqrt1_2 * fr[k];
      tw[2 * (off + a) + 1] = kJsSqrt1_2 * fi[k];
    }
    // SQRT1_2 * f_{w/2} (block-start pair) after the stage entries
    const size_t fq = (size_t)(L - 1) + (size_t)(__builtin_ctz((unsigned)w) - 1);
    tw[2 * fq] = kJsSqrt1_2 * fr[w / 2];
    tw[2 * fq + 1] = kJsSqrt1_2 * fi[w / 2];
    off += h;
  }
}

// Coefficients of the mixed butterflies (kernels.hip bfly_mixed_tame), same indexing as
// twiddles(): entry a > 0 of stage q holds (f_x, SQRT1_2 f_y) with f = f_{k(a)} unscaled;
// entry 0 (the block-start pair) holds (1, 0), so that fma(b, R, L) is exactly jsfft's
// left + right there; entry N/2 - 1 + q holds (f_{w/2,x}, SQRT1_2 f_{w/2,y}) (lane-uniform).
void mixed_coeffs(int n, std::vector<double>& tm) {
  const int L = n / 2;
  int stages = 0;
  for (int w = 2; w <= L; w <<= 1) ++stages;
  // 4 doubles per entry: (b, c0, t4, kL) (kernels.hip bfly_mixed_tame)
  tm.assign(4 * (size_t)(L - 1 + stages), 0.0);
  size_t off = 0;
  for (int w = 2; w <= L; w <<= 1) {
    const int h = w / 2;
    const double dr = cos(kJsPi / w), di = sin(kJsPi / w);
    std::vector<double> fr(w), fi(w);
    double r = 1, i = 0;
    for (int j = 0; j < w; j++) {
      fr[j] = r;
      fi[j] = i;
      const double t = r * dr - i * di;
      i = r * di + i * dr;
      r = t;
    }
    std::vector<int> kl;
    klist(w, kl);
    // block start: b = 1, c0 = 0, t4 = S f_y(w/2), kL = 0
    tm[4 * off] = 1.0;
    tm[4 * off + 2] = kJsSqrt1_2 * fi[w / 2];
    for (int a = 1; a < h; a++) {
      tm[4 * (off + a)] = fr[kl[a]];
      tm[4 * (off + a) + 1] = kJsSqrt1_2 * fi[kl[a]];
      tm[4 * (off + a) + 2] = kJsSqrt1_2 * fr[kl[a]];
      tm[4 * (off + a) + 3] = -kJsSqrt1_2;
    }
    const size_t fq = (size_t)(L - 1) + (size_t)(__builtin_ctz((unsigned)w) - 1);
    tm[4 * fq] = fr[w / 2];
    tm[4 * fq + 1] = kJsSqrt1_2 * fi[w / 2];
    off += h;
  }
}

// Mel filterbank as per-bin segment tables (kernels.hip mel_energies): bin k lies in
// segment m with b_m <= k < b_{m+1}, m in [0, nf]; band j rises over segment j and falls
// over segment j + 1 (mfcc.js:43-50). Bins at or past b_{nf+1} belong to no band.
void mel_segments(const int32_t* b, int nf, int L, std::vector<float>& wud, std::vector<uint8_t>& seg) {
  wud.assign(2 * (size_t)L, 0.0f);
  seg.assign(L, (uint8_t)(nf + 1));
  for (int k = 0; k < L; ++k) {
    int m = -1;
    for (int j = 0; j <= nf; ++j)
      if (b[j] <= k && k < b[j + 1]) m = j;
    if (m < 0) continue;
    seg[k] = (uint8_t)m;
    wud[2 * k] = (float)((double)(k - b[m]) / (b[m + 1] - b[m]));
    wud[2 * k + 1] = (float)((double)(b[m + 1] - k) / (b[m + 1] - b[m]));
  }
}

// Per-lane form of the segment tables for kernels.hip mel_energies (lane t owns bins
// [R t, R t + R), R = L / 64), one record of mgx::mel_rec_words(R) dwords per lane:
//   weights       per bin the rising weight and, up to R = 8, the falling one 1 - rising in
//                 float32 as a pair (the kernel forms it itself above)
//   R bytes       keep (1, or 0 where a segment starts: the sums restart)
//   8 bytes       keeps (0/1) of the 6 segmented-scan steps
//   2 words       the assembly offsets of band t (below)
// Dense layout of the wave's slot buffer (float2 (U, D) entries): lane t stores its running sums
// before bin jj >= 1 at entry (jj - 1) * 64 + t (fixed offsets, no per-bin address), the segmented
// scan's carry into it at (R - 1) * 64 + t, lane 63 the segment still open at the last bin at
// R * 64 and lane 0 a zero at R * 64 + 1. Segment m's total is carry-or-zero + entry: the running
// sum before the bin that starts the next segment (or the zero when that bin opens a lane), plus
// the carry into that lane when m began in an earlier lane; lane 63's inclusive scan value when m
// is open at the last bin; 0 when m has no bin. Band j (lane j < nf) sums U_j and D_{j+1} from the
// byte offsets (cU | dU << 16, cD | dD << 16). The scan keeps replay the flag logic of a
// Hillis-Steele segmented scan over the kernel's DPP steps (row_shr 1, 2, 4, 8; row_bcast 15 on
// rows 1, 3; row_bcast 31 on rows 2, 3), which depends only on which lanes hold a segment start.
void mel_lane_tables(const std::vector<uint8_t>& seg, const std::vector<float>& wud, int nf, int L,
                     std::vector<uint32_t>& rec) {
  const int R = L / 64, sink = nf + 1, W = mgx::mel_rec_words(R), B = (R + 3) / 4, WW = mgx::mel_weight_words(R);
  rec.assign((size_t)W * 64, 0u);
  const uint32_t zero = 8u * (uint32_t)(R * 64 + 1), tail = 8u * (uint32_t)(R * 64);
  bool seen[64];
  for (int t = 0; t < 64; ++t) {
    uint32_t* r = &rec[(size_t)W * t];
    uint8_t* keeps = reinterpret_cast<uint8_t*>(r + WW);
    seen[t] = false;
    for (int jj = 0; jj < R; ++jj) {
      const int k = R * t + jj;
      const int prevseg = k == 0 ? sink : seg[k - 1];
      const bool start = seg[k] != prevseg;
      if (start) seen[t] = true;
      keeps[jj] = start ? 0 : 1;
      if (WW == 2 * R) {  // (rise, 1 - rise): the falling weight the kernel would form, in float32
        const float up = wud[2 * k], dn = 1.0f - up;
        memcpy(&r[2 * jj], &up, 4);
        memcpy(&r[2 * jj + 1], &dn, 4);
      } else {
        memcpy(&r[jj], &wud[2 * k], 4);
      }
    }
  }
  // (carry-or-zero, entry) byte offsets of segment m's total
  auto total = [&](int m, uint32_t& c, uint32_t& d) {
    int first = -1, last = -1;
    for (int k = 0; k < L; ++k)
      if (seg[k] == m) {
        if (first < 0) first = k;
        last = k;
      }
    c = d = zero;
    if (first < 0) return;           // an empty segment: 0
    const int next = last + 1;
    if (next == L) {                 // open at the last bin: lane 63's inclusive scan value
      d = tail;
      return;
    }
    const int e = next / R, pos = next % R;
    if (first < e * R) c = 8u * (uint32_t)((R - 1) * 64 + e);  // started in an earlier lane: + its carry
    if (pos > 0) d = 8u * (uint32_t)((pos - 1) * 64 + e);       // the running sum before the next start
  };
  for (int j = 0; j < 64; ++j) {
    uint32_t cU = zero, dU = zero, cD = zero, dD = zero;
    if (j < nf) {
      total(j, cU, dU);
      total(j + 1, cD, dD);
    }
    uint32_t* r = &rec[(size_t)W * j];
    r[WW + B + 2] = cU | dU << 16;
    r[WW + B + 3] = cD | dD << 16;
  }
  bool f[64];
  for (int t = 0; t < 64; ++t) f[t] = seen[t];
  for (int s = 0; s < 6; ++s) {
    bool g[64];
    for (int t = 0; t < 64; ++t) {
      const int row = t / 16;
      int src = -1;
      if (s < 4) src = (t % 16) >= (1 << s) ? t - (1 << s) : -1;
      else if (s == 4) src = (row == 1 || row == 3) ? row * 16 - 1 : -1;
      else src = (row == 2 || row == 3) ? 31 : -1;
      uint8_t* lane8 = reinterpret_cast<uint8_t*>(&rec[(size_t)W * t + WW + B]);
      // 0 also where the step has no source for this lane: the kernel's row broadcasts write
      // every row (no row mask), so a row outside the step's rows must not add what it receives
      lane8[s] = (f[t] || src < 0) ? 0 : 1;
      g[t] = f[t] || (src >= 0 && f[src]);
    }
    memcpy(f, g, sizeof f);
  }
}

// MGX_FLAG_MFCC_REFERENCE: the mel band sums of mfcc.js:53-62 in the reference's
// own order, as serial chains (kernels.hip mel_chains). Band j's chain walks its bins
// [b_j, b_{j+2}) (clamped to the reference's j < N/2) in ascending order with the weights of
// mfcc.js:43-50 -- (k - b_j) / (b_{j+1} - b_j) rising, (b_{j+2} - k) / (b_{j+2} - b_{j+1}) falling,
// IEEE double quotients as JavaScript forms them -- and the float32 accumulator (every other bin
// adds an exact +0 in the reference for a finite spectrum). F frames x nf such chains run together
// (F = 8: two consecutive batches of a wave, when nf <= kChainPairMaxMel; else the batch's 4).
// A chain runs in whole groups of 8 steps from its first bin rounded down to 4 (16-byte row loads),
// or earlier if it would run past N/2, with leading zero weights (a zero weight times a finite
// power adds +0); a band without bins (low bands of many-band plans) has one group of zero
// weights, so its energy is the reference's 0.
// Packed tracks: the 64 lanes are 64 / F tracks x the F frames (lane = track * F + frame). The
// bands are dealt to the tracks longest first, each to the least loaded track, and a track runs its
// bands' chains back to back, so the lanes stay busy for ngroups = the largest track load (N = 1024,
// 26 bands: 18 groups instead of the 24 of phases whose length is the phase's longest chain).
//   ctl[g * 64 + lane], g < ngroups (the lane's row and what happens at the group's start):
//     bits 0-12 the row offset in floats (frame * L + bin), bit 25 a chain starts here (its first
//     step adds to 0), bit 26 the finished chain before it is
//     stored at bits 13-24 (a byte offset into the wave's frame records: FrameRec::lm of its frame
//     and band); without bit 26 the store goes to the lane's scratch word.
//   ctl[ngroups * 64 + lane]: the store of the lane's last chain (bit 26 and bits 13-24 only).
//   w[track * ngroups * 8 + s]: the weight of the track's step s (0 past its last chain).
struct ChainSched {
  int ngroups = 0;
  std::vector<uint32_t> ctl;
  std::vector<double> w;
};
// (the control word's fields hold every plan: 8 frames' rows at N = kChainMaxN, the last record's lm[63])
static_assert(8 * (mgx::kChainMaxN / 2) - 1 <= 0x1FFF, "row offsets fit bits 0-12");
static_assert(3 * mgx::kRecBytes + mgx::kRecLmOff + 4 * (mgx::kMaxMel - 1) <= 0xFFF, "record offsets fit bits 13-24");
void chain_schedule(const int32_t* b, int nf, int L, int F, ChainSched& cs) {
  const int ntr = 64 / F;
  std::vector<int> lo(nf), len(nf), order;
  for (int j = 0; j < nf; ++j) {
    const int first = std::min<int>(b[j], L), end = std::min<int>(b[j + 2], L);
    lo[j] = first / 4 * 4;
    len[j] = std::max(8, (std::max(0, end - lo[j]) + 7) / 8 * 8);
    if (lo[j] + len[j] > L) lo[j] = L - len[j];  // (L and len multiples of 8)
    order.push_back(j);
  }
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return len[x] > len[y]; });
  std::vector<std::vector<int>> track(ntr);
  std::vector<int> load(ntr, 0);
  for (int j : order) {
    int t = 0;
    for (int u = 1; u < ntr; ++u)
      if (load[u] < load[t]) t = u;
    track[t].push_back(j);
    load[t] += len[j];
  }
  const int ng = *std::max_element(load.begin(), load.end()) / 8;
  cs.ngroups = ng;
  cs.ctl.assign((size_t)(ng + 1) * 64, 0u);
  cs.w.assign((size_t)ntr * ng * 8, 0.0);
  auto target = [&](int j, int f) {  // byte offset of FrameRec::lm[band (+32: a pair's first batch)]
    const int lmo = (F == 8 && f < 4) ? 32 : 0;
    return (uint32_t)((f & 3) * mgx::kRecBytes + mgx::kRecLmOff + 4 * (j + lmo)) << 13 | 1u << 26;
  };
  for (int t = 0; t < ntr; ++t) {
    double* w = cs.w.data() + (size_t)t * ng * 8;
    int g0 = 0;
    for (size_t c = 0; c < track[t].size(); ++c) {
      const int j = track[t][c];
      for (int s = 0; s < len[j]; ++s) {
        const int k = lo[j] + s;
        double v = 0.0;
        if (k >= b[j] && k < b[j + 1] && k < L) v = (double)(k - b[j]) / (double)(b[j + 1] - b[j]);
        else if (k >= b[j + 1] && k < b[j + 2] && k < L) v = (double)(b[j + 2] - k) / (double)(b[j + 2] - b[j + 1]);
        w[g0 * 8 + s] = v;
      }
      for (int f = 0; f < F; ++f) {
        const int lane = t * F + f;
        for (int g = g0; g < g0 + len[j] / 8; ++g) {
          uint32_t c32 = (uint32_t)(f * L + lo[j] + 8 * (g - g0));
          if (g == g0) c32 |= 1u << 25 | (c > 0 ? target(track[t][c - 1], f) : 0u);
          cs.ctl[(size_t)g * 64 + lane] = c32;
        }
      }
      g0 += len[j] / 8;
    }
    for (int f = 0; f < F; ++f) {
      const int lane = t * F + f;
      // past the track's last chain: bin 0 of the frame with zero weights (adds +0); no reset
      for (int g = g0; g < ng; ++g) cs.ctl[(size_t)g * 64 + lane] = (uint32_t)(f * L);
      cs.ctl[(size_t)ng * 64 + lane] = track[t].empty() ? 0u : target(track[t].back(), f);
    }
  }
}

int validate(const mgx_plan_desc* d) {
  if (!d) return fail(MGX_E_INVALID_ARGUMENT, "plan descriptor is NULL");
  if (d->struct_size != sizeof(mgx_plan_desc))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_plan_desc.struct_size is %u, expected %zu", d->struct_size, sizeof(mgx_plan_desc));
  if (!mgx_is_power_of_two((double)d->buffer_size))
    return fail(MGX_E_NOT_POWER_OF_TWO, "Buffer size is not a power of two: Meyda will not run.");
  if (!(d->sample_rate > 0) || !std::isfinite(d->sample_rate))
    return fail(MGX_E_INVALID_ARGUMENT, "sample_rate must be positive and finite");
  if (d->window > MGX_WINDOW_HAMMING) return fail(MGX_E_INVALID_ARGUMENT, "unknown window %u", d->window);
  if (d->precision > MGX_PRECISION_FAST) return fail(MGX_E_INVALID_ARGUMENT, "unknown precision %u", d->precision);
  if (d->mode > MGX_MODE_LITERAL) return fail(MGX_E_INVALID_ARGUMENT, "unknown mode %u", d->mode);
  if (d->num_bark_bands != mgx::kBark) return fail(MGX_E_UNSUPPORTED, "num_bark_bands must be 24 (loudness.js)");
  if (d->num_mel_bands < 1 || d->num_mel_bands > (uint32_t)mgx::kMaxMel)
    return fail(MGX_E_UNSUPPORTED, "num_mel_bands must be in [1, %d]", mgx::kMaxMel);
  if (d->num_mfcc_coeffs < 1 || d->num_mfcc_coeffs > (uint32_t)mgx::kMaxCoeffs)
    return fail(MGX_E_UNSUPPORTED, "num_mfcc_coeffs must be in [1, %d]", mgx::kMaxCoeffs);
  if (d->flags & ~(MGX_FLAG_DCT_SEQUENTIAL | MGX_FLAG_MFCC_REFERENCE | MGX_FLAG_RESIDENT)) return fail(MGX_E_INVALID_ARGUMENT, "unknown plan flags 0x%x", d->flags);
  return MGX_OK;
}

template <typename T>
size_t carve(size_t& off, size_t count) {
  off = (off + 255) / 256 * 256;
  const size_t at = off;
  off += count * sizeof(T);
  return at;
}

}  // namespace

struct mgx_plan {
  mgx_plan_desc d;
  int n = 0, L = 0;
  unsigned char* dev = nullptr;
  void* lds_image = nullptr;  // DevTables::lds_image (its own allocation)
  mgx::DevTables t{};
  double freq_sum = 0, pow_freq_sum = 0, nyq = 0, sharp_tail = 0;
  int grid_cap = 1;
  int cus = 0;  // compute units of the plan's device
  int chain_groups = 0;  // MGX_FLAG_MFCC_REFERENCE: 8-step groups of the mel chains (chain_schedule)
  int chain_pair = 0;  // ... over two consecutive batches of a wave (8 frames)
  // Per-stream device scratch, one set per stream a launch used (the launches of one stream run
  // in order, those of two streams may overlap): the scalar windows (kernels.hip scalar_pass) and,
  // for the reference-order MFCC, the mel chains' power rows (mel_chains). Each set's event is
  // recorded after every launch that uses it, so destroy waits for exactly those launches (the
  // stream itself may be gone by then).
  struct ChainRing {
    void* stream;
    uint64_t* scal;
    float* rows;  // null until a reference-order MFCC launch on the stream
    hipEvent_t done;
    uint64_t* pool_ctr = nullptr;  // the tail pool's ticket counter (KernelArgs::pool_ctr; N = 2048 plans)
  };
  std::vector<ChainRing> chain_rings;
  // two device slots for mgx_extract_host (copy of chunk i+1 beside the extraction of chunk i)
  float* s_frames[2] = {nullptr, nullptr};
  unsigned char* s_out[2] = {nullptr, nullptr};
  size_t s_out_bytes = 0;
  uint64_t s_chunk = 0;
  unsigned char* s_pcm[2] = {nullptr, nullptr};  // raw PCM slots for mgx_extract_host_pcm
  uint64_t* s_starts[2] = {nullptr, nullptr};    // a chunk's starts for mgx_extract_gather_host (kHostChunk entries each)
  uint64_t s_pcm_bytes = 0;
  // mgx_summarize_host: the table, the shifts, the partials and the summaries themselves on the device (one
  // allocation, grown when a call needs more)
  unsigned char* s_sum = nullptr;
  size_t s_sum_bytes = 0;
  // mgx_summarize_deltas_host: the delta'd fields' rows of the whole call, their delta and second-order rows, a
  // table, shifts, partials and summaries of their own (one allocation beside s_sum, grown when a call needs more)
  unsigned char* s_delta = nullptr;
  size_t s_delta_bytes = 0;
  // mgx_summarize_flux_host: a table, per request the two carries of lag rows and the flux column of the whole
  // call, then shifts, partials and summaries (one allocation, grown when a call needs more); mgx_onsets_host: behind
  // them the picker's workspace, its offsets and the peaks the caller has room for
  unsigned char* s_flux = nullptr;
  size_t s_flux_bytes = 0;
  // mgx_chroma_host: the bank, the chroma rows of the whole call, then a table, shifts, partials and summaries (one
  // allocation, grown when a call needs more)
  unsigned char* s_chroma = nullptr;
  size_t s_chroma_bytes = 0;
  // mgx_hpss_host: the call's amplitude rows, the two parts and what the requests behind them need
  unsigned char* s_hpss = nullptr;
  size_t s_hpss_bytes = 0;
  // mgx_tempo_host: the window, the prior, the workspace of mgx_tempo_device and the lags (one allocation, grown
  // when a call needs more)
  unsigned char* s_tempo = nullptr;
  size_t s_tempo_bytes = 0;
  hipStream_t s_copy = nullptr, s_comp = nullptr;
  hipEvent_t ev_loaded[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}, ev_back[2] = {nullptr, nullptr};
  // small host batches (kSmallBatchFrames): pinned, device-mapped, coherent host buffers
  uint64_t small_max = kSmallBatchFrames;
  int pool_pct = 15;  // the N = 2048 tail pool's share of the groups, percent (MGX_POOL_PCT overrides; 0: off)
  // a launch whose frames exceed this many bytes reads them with non-temporal loads (KernelArgs::nt_frames):
  // the MALL's 256 MiB (MGX_NT_MIN_MB overrides, in MiB)
  uint64_t nt_min_bytes = 256ull << 20;
  bool nt_forced = false;  // MGX_NT_MIN_MB was given: it also decides for overlapping frames (plain by default)
  // the small path's completion word (KernelArgs::done_flag): a mapped host word, the device
  // counter of finished waves and the launch sequence number
  uint32_t* h_done = nullptr;
  // the device addresses of h_in, h_out and h_done (looked up once per allocation, not per call)
  void* d_in_map = nullptr;
  void* d_out_map = nullptr;
  uint32_t* d_done_map = nullptr;
  uint32_t* d_done_count = nullptr;
  uint32_t done_seq = 0;
  float* h_in = nullptr;
  unsigned char* h_out = nullptr;
  size_t h_in_bytes = 0, h_out_bytes = 0;
  // MGX_FLAG_RESIDENT: one-frame host calls served by a launch that stays on the device (resident_request)
  bool resident = false;
  uint32_t res_idle_ms = 20;   // its idle timeout (MGX_RESIDENT_IDLE_MS overrides)
  bool res_light = false;      // MGX_RESIDENT_POLL=light: the launch polls the first word only (kernels.hip res_wait)
  hipStream_t s_res = nullptr; // its own stream: nothing else is queued behind it
  uint64_t* h_mail = nullptr;  // pinned, mapped: N request words (KernelArgs::res_mail), then the exit word
  uint64_t* d_mail = nullptr;  // the device address of h_mail
  bool res_live = false;       // a resident launch was started and has not been seen to end
  uint32_t res_key = 0;        // the outputs it writes (bit k: output k of mgx_outputs requested)
  uint32_t res_next = 0;       // the request number it waits for next
};

namespace {
// resident: the launch is the plan's resident server (MGX_FLAG_RESIDENT), serving requests seq, seq + 1, ...
struct ResidentLaunch {
  uint32_t seq;
};
// gather: the launch's frames start where a table says (mgx_extract_gather_*): starts, nframes entries in device
// memory, into the num_samples samples at `frames`
struct GatherLaunch {
  const uint64_t* starts;
  uint64_t num_samples;
};
// What a launch may carry beyond its frames and outputs (extract_device_impl), each null when it does not
struct LaunchOpts {
  const uint32_t* done = nullptr;         // the small host path's completion word (device address)
  const float* inline_frame = nullptr;    // the small path's one frame in host memory, for the kernel arguments
  const ResidentLaunch* res = nullptr;
  const GatherLaunch* gather = nullptr;
};
int extract_device_impl(mgx_plan* p, const float* frames, uint64_t nframes, uint64_t stride, const mgx::Outputs* o, void* stream,
                        const LaunchOpts& opt = LaunchOpts{});
void resident_stop(mgx_plan* p);

// The plan's entry in the per-device tables (g_resident_live)
int dev_slot(const mgx_plan* p) { return p->d.device >= 0 && p->d.device < kMaxDevices ? p->d.device : 0; }

// What every mgx_extract_* entry point begins with: the plan and the outputs are there, and the caller's two
// output structs become the one the plan code passes around. aux: NULL (no output beyond mgx_outputs), or a
// mgx_aux_outputs of exactly this build's size -- the check that lets the struct grow.
int make_outputs(const mgx_plan* p, const mgx_outputs* o, const mgx_aux_outputs* aux, mgx::Outputs* out) {
  if (!p || !o) return fail(MGX_E_INVALID_ARGUMENT, "NULL plan or outputs");
  *out = mgx::from_public(*o);
  if (!aux) return MGX_OK;
  if (aux->struct_size != sizeof(mgx_aux_outputs))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_aux_outputs.struct_size is %u, expected %zu", aux->struct_size, sizeof(mgx_aux_outputs));
  if (aux->reserved != 0) return fail(MGX_E_INVALID_ARGUMENT, "mgx_aux_outputs.reserved is %u, expected 0", aux->reserved);
  out->mel_bands = aux->mel_bands;
  return MGX_OK;
}

// The rule about the outputs themselves (mgx::outputs_ok) as an error. Each kind of call reports it where it
// always has among its argument errors: after the empty call and the NULL inputs (for PCM before them).
int check_outputs(const mgx::Outputs& o) {
  const char* why = nullptr;
  const int rc = mgx::outputs_ok(o, &why);
  return rc ? fail(rc, "%s", why) : MGX_OK;
}
}  // namespace

extern "C" {

int mgx_abi_version(void) { return MGX_ABI_VERSION; }
const char* mgx_last_error(void) { return g_last_error.c_str(); }

// src/utils.js:13-19
int mgx_is_power_of_two(double num) {
  while (fmod(num, 2.0) == 0.0 && num > 1) num /= 2;
  return num == 1;
}

int mgx_feature_index(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < MGX_NUM_FEATURES; ++i)
    if (strcmp(name, kNames[i]) == 0) return i;
  return -1;
}
const char* mgx_feature_name(int f) { return (f >= 0 && f < MGX_NUM_FEATURES) ? kNames[f] : nullptr; }
int mgx_feature_info(int f) { return (f >= 0 && f < MGX_NUM_FEATURES) ? kInfo[f] : -1; }

void mgx_plan_desc_init(mgx_plan_desc* d) {
  if (!d) return;
  memset(d, 0, sizeof *d);
  d->struct_size = sizeof *d;
  d->buffer_size = 512;
  d->sample_rate = 44100.0;
  d->window = MGX_WINDOW_HANNING;
  d->precision = MGX_PRECISION_FAITHFUL;
  d->mode = MGX_MODE_PER_BUFFER_FFT;
  d->num_bark_bands = 24;
  d->num_mel_bands = 26;
  d->num_mfcc_coeffs = 13;
  d->scalar_f64 = 0;
  d->device = 0;
}

int mgx_device_count(int* count) {
  if (!count) return fail(MGX_E_INVALID_ARGUMENT, "count is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) c = 0;
  *count = c;
  return MGX_OK;
}

int mgx_get_host_tables(const mgx_plan_desc* d, const mgx_host_tables* out) {
  int rc = validate(d);
  if (rc) return rc;
  if (!out) return fail(MGX_E_INVALID_ARGUMENT, "tables is NULL");
  const int n = (int)d->buffer_size, nf = (int)d->num_mel_bands, nc = (int)d->num_mfcc_coeffs;
  std::vector<float> han(n), ham(n), bark(n);
  hanning(n, han.data());
  hamming(n, ham.data());
  bark_scale(n, d->sample_rate, bark.data());
  if (out->hanning) memcpy(out->hanning, han.data(), n * sizeof(float));
  if (out->hamming) memcpy(out->hamming, ham.data(), n * sizeof(float));
  if (out->window) memcpy(out->window, d->window == MGX_WINDOW_HAMMING ? ham.data() : han.data(), n * sizeof(float));
  if (out->bark_scale) memcpy(out->bark_scale, bark.data(), n * sizeof(float));
  if (out->bark_limits) bark_limits(bark.data(), n / 2, mgx::kBark, out->bark_limits);
  if (out->mel_bins) mel_bins(n, d->sample_rate, nf, out->mel_bins);
  if (out->dct) dct_table(nf, nc, out->dct);
  return MGX_OK;
}

int mgx_plan_create(const mgx_plan_desc* d, mgx_plan** out) {
  if (!out) return fail(MGX_E_INVALID_ARGUMENT, "out_plan is NULL");
  *out = nullptr;
  int rc = validate(d);
  if (rc) return rc;
  const int n = (int)d->buffer_size;
  if (n < 256 || n > 4096)
    return fail(MGX_E_UNSUPPORTED, "buffer_size %d: the GPU path supports 256..4096", n);
  // The two plan kinds without a 4096 form, refused here (ahead of the device, as the range) rather than
  // dropped: the reference-order chains' control word holds row offsets up to N = kChainMaxN (chain_schedule),
  // and the resident wait's two mailbox reads in flight do not fit the registers above kResidentMaxN.
  if ((d->flags & MGX_FLAG_MFCC_REFERENCE) && n > mgx::kChainMaxN)
    return fail(MGX_E_UNSUPPORTED, "MGX_FLAG_MFCC_REFERENCE: not at buffer_size %d (up to %d)", n, mgx::kChainMaxN);
  if ((d->flags & MGX_FLAG_RESIDENT) && n > mgx::kResidentMaxN)
    return fail(MGX_E_UNSUPPORTED, "MGX_FLAG_RESIDENT: not at buffer_size %d (up to %d)", n, mgx::kResidentMaxN);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MGX_E_NO_DEVICE, "no HIP device available");
  if (d->device < 0 || d->device >= ndev) return fail(MGX_E_INVALID_ARGUMENT, "device %d out of range (%d devices)", d->device, ndev);
  hipError_t e = hipSetDevice(d->device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, d->device);
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(MGX_E_NO_DEVICE, "device %d is %s; this build targets gfx950 (MI355X)", d->device, prop.gcnArchName);

  const int L = n / 2, nf = (int)d->num_mel_bands, nc = (int)d->num_mfcc_coeffs;
  std::vector<float> han(n), ham(n), bark(n), dct((size_t)nc * nf);
  hanning(n, han.data());
  hamming(n, ham.data());
  bark_scale(n, d->sample_rate, bark.data());
  int32_t lim[mgx::kBark + 1];
  bark_limits(bark.data(), L, mgx::kBark, lim);
  std::vector<int32_t> bins(nf + 2);
  mel_bins(n, d->sample_rate, nf, bins.data());
  dct_table(nf, nc, dct.data());
  std::vector<double> tw;
  twiddles(n, tw);
  std::vector<double> twm;
  mixed_coeffs(n, twm);
  std::vector<float> twf(tw.size());
  for (size_t i = 0; i < tw.size(); ++i) twf[i] = (float)tw[i];
  std::vector<int> kl;
  klist(n, kl);
  std::vector<float> mwud;
  std::vector<uint8_t> mseg;
  mel_segments(bins.data(), nf, L, mwud, mseg);
  std::vector<uint32_t> mrec;
  mel_lane_tables(mseg, mwud, nf, L, mrec);
  const bool chain = (d->flags & MGX_FLAG_MFCC_REFERENCE) && d->mode == MGX_MODE_PER_BUFFER_FFT &&
                     d->precision == MGX_PRECISION_FAITHFUL && n <= mgx::kChainMaxN;
  ChainSched cs;
  const bool pair = chain && nf <= mgx::kChainPairMaxMel;
  if (chain) chain_schedule(bins.data(), nf, L, pair ? 8 : 4, cs);

  if ((d->flags & MGX_FLAG_RESIDENT) && (d->precision != MGX_PRECISION_FAITHFUL || d->mode != MGX_MODE_PER_BUFFER_FFT || chain))
    return fail(MGX_E_UNSUPPORTED, "MGX_FLAG_RESIDENT: faithful per-buffer plans without MGX_FLAG_MFCC_REFERENCE only");

  auto* p = new mgx_plan();
  p->d = *d;
  p->resident = (d->flags & MGX_FLAG_RESIDENT) != 0;
  p->n = n;
  p->L = L;
  // spectralSlope.js:9-16 input-independent sums, in the reference's order
  for (int i = 0; i < L; i++) {
    const double f = (double)i * d->sample_rate / n;
    p->pow_freq_sum += f * f;
    p->freq_sum += f;
  }
  p->nyq = d->sample_rate / (2.0 * (L - 1));  // spectralRolloff.js:4
  for (int i = 15; i < mgx::kBark; ++i) p->sharp_tail += 0.066 * exp(0.171 * (i + 1));  // perceptualSharpness.js:10
  // persistent grid: exactly the workgroups that are resident at once
  p->grid_cap = prop.multiProcessorCount * std::max(1, mgx::extract_blocks_per_cu(n, (int)d->precision, (int)d->mode, (int)d->num_mfcc_coeffs, (int)d->num_mel_bands, chain));
  p->chain_groups = cs.ngroups;
  p->chain_pair = pair;
  p->cus = prop.multiProcessorCount;
  // (tuning knob: MGX_GRID_CAP overrides the persistent grid's size; MGX_GRID_CAP=print reports it)
  if (const char* gc = getenv("MGX_GRID_CAP")) {
    if (strcmp(gc, "print") == 0) fprintf(stderr, "mgx: grid_cap %d (%d CUs)\n", p->grid_cap, prop.multiProcessorCount);
    else if (atoi(gc) > 0) p->grid_cap = atoi(gc);
  }
  if (const char* sb = getenv("MGX_SMALL_BATCH_FRAMES")) p->small_max = (uint64_t)std::max(0, atoi(sb));
  if (const char* pp = getenv("MGX_POOL_PCT")) p->pool_pct = std::min(50, std::max(0, atoi(pp)));
  if (const char* nm = getenv("MGX_NT_MIN_MB")) {
    p->nt_min_bytes = (uint64_t)std::max(0, atoi(nm)) << 20;
    p->nt_forced = true;
  }
  if (const char* ri = getenv("MGX_RESIDENT_IDLE_MS")) p->res_idle_ms = (uint32_t)std::min(10000, std::max(1, atoi(ri)));
  if (const char* rp = getenv("MGX_RESIDENT_POLL")) p->res_light = strcmp(rp, "light") == 0;

  size_t off = 0;
  const size_t o_win = carve<float>(off, n), o_tw = carve<double>(off, tw.size()),
               o_twf = carve<float>(off, twf.size()), o_twm = carve<double>(off, twm.size()),
               o_kl = carve<int>(off, L),
               o_lim = carve<int>(off, mgx::kBark + 1), o_mw = carve<uint32_t>(off, mrec.size()), o_dct = carve<float>(off, dct.size()),
               o_mb = carve<int32_t>(off, bins.size()), o_cl = carve<uint32_t>(off, cs.ctl.size()),
               o_cw = carve<double>(off, cs.w.size()), o_lt = carve<double>(off, 2 * 64);
  std::vector<unsigned char> host(off, 0);
  auto put = [&](size_t at, const void* src, size_t bytes) { if (bytes) memcpy(host.data() + at, src, bytes); };
  put(o_win, d->window == MGX_WINDOW_HAMMING ? ham.data() : han.data(), n * sizeof(float));
  put(o_tw, tw.data(), tw.size() * sizeof(double));
  put(o_twf, twf.data(), twf.size() * sizeof(float));
  put(o_twm, twm.data(), twm.size() * sizeof(double));
  put(o_kl, kl.data(), L * sizeof(int));
  put(o_lim, lim, sizeof lim);
  put(o_mw, mrec.data(), mrec.size() * sizeof(uint32_t));
  put(o_mb, bins.data(), bins.size() * sizeof(int32_t));
  put(o_dct, dct.data(), dct.size() * sizeof(float));
  put(o_cl, cs.ctl.data(), cs.ctl.size() * sizeof(uint32_t));
  put(o_cw, cs.w.data(), cs.w.size() * sizeof(double));
  {
    // the reference-order MFCC's natural log (kernels.hip ref_ln): per 1/64 of the mantissa range its centre's
    // reciprocal, rounded, and the negated log of that reciprocal, from the 64-bit-mantissa long double log
    double lt[2 * 64];
    for (int k = 0; k < 64; ++k) {
      const double inv = (double)(1.0L / (1.0L + (long double)(2 * k + 1) / 128.0L));
      lt[2 * k] = inv;
      lt[2 * k + 1] = (double)(-logl((long double)inv));
    }
    put(o_lt, lt, sizeof lt);
  }
  e = hipMalloc(reinterpret_cast<void**>(&p->dev), off);
  if (e != hipSuccess) { delete p; return hip_fail(e, "hipMalloc(plan tables)"); }
  e = hipMemcpy(p->dev, host.data(), off, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(p->dev); delete p; return hip_fail(e, "hipMemcpy(plan tables)"); }
  unsigned char* b = p->dev;
  p->t.window = reinterpret_cast<const float*>(b + o_win);
  p->t.tw = reinterpret_cast<const double2*>(b + o_tw);
  p->t.twf = reinterpret_cast<const float2*>(b + o_twf);
  p->t.twm = reinterpret_cast<const double2*>(b + o_twm);
  p->t.klist = reinterpret_cast<const int*>(b + o_kl);
  p->t.bblim = reinterpret_cast<const int*>(b + o_lim);
  p->t.mel_rec = reinterpret_cast<const uint32_t*>(b + o_mw);
  p->t.mel_bins = reinterpret_cast<const int*>(b + o_mb);
  p->t.dct = reinterpret_cast<const float*>(b + o_dct);
  p->t.chain_ctl = reinterpret_cast<const uint32_t*>(b + o_cl);
  p->t.chain_w = reinterpret_cast<const double*>(b + o_cw);
  p->t.log_tab = reinterpret_cast<const double2*>(b + o_lt);
  // the workgroup's LDS tables as one image (kernels.hip lds_image_kernel), built here once
  {
    const size_t ib = mgx::lds_image_bytes(n, nc, nf);
    mgx::KernelArgs ia{};
    ia.t = p->t;
    ia.nfilt = nf;
    ia.ncoef = nc;
    e = hipMalloc(&p->lds_image, ib);
    if (e == hipSuccess) e = hipMemset(p->lds_image, 0, ib);
    if (e == hipSuccess) e = mgx::launch_lds_image(n, (int)d->precision, (int)d->mode, ia, p->lds_image, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
      if (p->lds_image) (void)hipFree(p->lds_image);
      (void)hipFree(p->dev);
      delete p;
      return hip_fail(e, "plan LDS image");
    }
    p->t.lds_image = p->lds_image;
    p->t.lds_image_chunks = (uint32_t)(ib / 16);
  }
  if (p->resident) {
    // The resident path's one-time set-up here instead of in the first real-time call, where it took ~13 ms
    // (the pinned buffers, the CU-masked stream's hardware queue; profiles/r06_resident.txt): one call on a
    // silent frame with every output (the largest layout), then the launch is ended.
    std::vector<float> z((size_t)n, 0.0f);
    uint64_t at[mgx::kOutFields];
    std::vector<unsigned char> buf(mgx::out_layout(*d, mgx::kGroupFieldBits, 1, at));
    const mgx_outputs o = mgx::public_part(mgx::out_at(buf.data(), at));
    int rc = mgx_extract_host(p, z.data(), 1, &o);
    resident_stop(p);
    if (rc) {
      const std::string why = g_last_error;
      mgx_plan_destroy(p);
      return fail(rc, "MGX_FLAG_RESIDENT set-up: %s", why.c_str());
    }
  }
  *out = p;
  return MGX_OK;
}

int mgx_plan_destroy(mgx_plan* p) {
  if (!p) return MGX_OK;
  (void)hipSetDevice(p->d.device);
  // the resident launch ends first (its stop word, then its stream)
  resident_stop(p);
  // every launch that used the plan's memory is done first: the plan's own streams, then the
  // caller streams' scratch events (launches on s_comp record none)
  if (p->s_copy) (void)hipStreamSynchronize(p->s_copy);
  if (p->s_comp) (void)hipStreamSynchronize(p->s_comp);
  for (auto& r : p->chain_rings) (void)hipEventSynchronize(r.done);
  if (p->dev) (void)hipFree(p->dev);
  if (p->lds_image) (void)hipFree(p->lds_image);
  for (auto& r : p->chain_rings) {
    (void)hipEventDestroy(r.done);
    if (r.scal) (void)hipFree(r.scal);
    if (r.rows) (void)hipFree(r.rows);
    if (r.pool_ctr) (void)hipFree(r.pool_ctr);
  }
  for (int i = 0; i < 2; ++i) {
    if (p->s_frames[i]) (void)hipFree(p->s_frames[i]);
    if (p->s_out[i]) (void)hipFree(p->s_out[i]);
    if (p->s_pcm[i]) (void)hipFree(p->s_pcm[i]);
    if (p->s_starts[i]) (void)hipFree(p->s_starts[i]);
    for (hipEvent_t ev : {p->ev_loaded[i], p->ev_done[i], p->ev_back[i]})
      if (ev) (void)hipEventDestroy(ev);
  }
  if (p->s_sum) (void)hipFree(p->s_sum);
  if (p->s_delta) (void)hipFree(p->s_delta);
  if (p->s_flux) (void)hipFree(p->s_flux);
  if (p->s_chroma) (void)hipFree(p->s_chroma);
  if (p->s_hpss) (void)hipFree(p->s_hpss);
  if (p->s_tempo) (void)hipFree(p->s_tempo);
  if (p->s_copy) (void)hipStreamDestroy(p->s_copy);
  if (p->s_comp) (void)hipStreamDestroy(p->s_comp);
  if (p->s_res) (void)hipStreamDestroy(p->s_res);
  if (p->h_mail) (void)hipHostFree(p->h_mail);
  if (p->h_in) (void)hipHostFree(p->h_in);
  if (p->h_out) (void)hipHostFree(p->h_out);
  if (p->h_done) (void)hipHostFree(p->h_done);
  if (p->d_done_count) (void)hipFree(p->d_done_count);
  delete p;
  return MGX_OK;
}

int mgx_plan_get_desc(const mgx_plan* p, mgx_plan_desc* out) {
  if (!p || !out) return fail(MGX_E_INVALID_ARGUMENT, "NULL argument");
  *out = p->d;
  return MGX_OK;
}

int mgx_extract_device(mgx_plan* p, const float* frames, uint64_t nframes, const mgx_outputs* o, void* stream) {
  if (!p || !o) return fail(MGX_E_INVALID_ARGUMENT, "NULL plan or outputs");
  return mgx_extract_device_ex(p, frames, nframes * (uint64_t)p->n, (uint32_t)p->n, o, nullptr, stream);
}

// src/meyda.js:69-91 delivers disjoint buffers; with a hop the same buffers start every `hop` samples
int mgx_signal_frames(uint64_t num_samples, uint32_t buffer_size, uint32_t hop, uint64_t* num_frames) {
  if (!num_frames) return fail(MGX_E_INVALID_ARGUMENT, "num_frames is NULL");
  if (buffer_size == 0) return fail(MGX_E_INVALID_ARGUMENT, "buffer_size is 0");
  if (hop == 0) return fail(MGX_E_INVALID_ARGUMENT, "hop is 0 (a hop of at least one sample)");
  *num_frames = num_samples < buffer_size ? 0 : (num_samples - buffer_size) / hop + 1;
  return MGX_OK;
}

int mgx_extract_signal_device(mgx_plan* p, const float* samples, uint64_t num_samples, uint32_t hop, const mgx_outputs* o,
                              void* stream) {
  return mgx_extract_device_ex(p, samples, num_samples, hop, o, nullptr, stream);
}

int mgx_extract_device_ex(mgx_plan* p, const float* samples, uint64_t num_samples, uint32_t hop, const mgx_outputs* o,
                          const mgx_aux_outputs* aux, void* stream) {
  mgx::Outputs x;
  int rc = make_outputs(p, o, aux, &x);
  if (rc) return rc;
  uint64_t nframes = 0;
  rc = mgx_signal_frames(num_samples, (uint32_t)p->n, hop, &nframes);
  if (rc) return rc;
  return extract_device_impl(p, samples, nframes, hop, &x, stream);
}

// A corpus as one array: the buffers of every signal, none across a signal's end
int mgx_signals_frame_starts(const uint64_t* offsets, uint64_t num_signals, uint32_t buffer_size, uint32_t hop,
                             uint64_t* frame_offsets, uint64_t* starts, uint64_t capacity, uint64_t* num_frames) {
  if (!num_frames) return fail(MGX_E_INVALID_ARGUMENT, "num_frames is NULL");
  if (buffer_size == 0) return fail(MGX_E_INVALID_ARGUMENT, "buffer_size is 0");
  if (hop == 0) return fail(MGX_E_INVALID_ARGUMENT, "hop is 0 (a hop of at least one sample)");
  if (!offsets) return fail(MGX_E_INVALID_ARGUMENT, "offsets is NULL");
  uint64_t total = 0;
  for (uint64_t s = 0; s < num_signals; ++s) {
    if (offsets[s + 1] < offsets[s])
      return fail(MGX_E_INVALID_ARGUMENT, "offsets[%llu] = %llu is below offsets[%llu] = %llu", (unsigned long long)(s + 1),
                  (unsigned long long)offsets[s + 1], (unsigned long long)s, (unsigned long long)offsets[s]);
    const uint64_t len = offsets[s + 1] - offsets[s];
    total += len < buffer_size ? 0 : (len - buffer_size) / hop + 1;
  }
  if (starts && capacity < total)
    return fail(MGX_E_INVALID_ARGUMENT, "starts holds %llu entries, %llu buffers", (unsigned long long)capacity, (unsigned long long)total);
  // (nothing is written before every check has passed)
  uint64_t at = 0;
  for (uint64_t s = 0; s < num_signals; ++s) {
    if (frame_offsets) frame_offsets[s] = at;
    const uint64_t len = offsets[s + 1] - offsets[s];
    const uint64_t k = len < buffer_size ? 0 : (len - buffer_size) / hop + 1;
    for (uint64_t i = 0; starts && i < k; ++i) starts[at + i] = offsets[s] + i * hop;
    at += k;
  }
  if (frame_offsets) frame_offsets[num_signals] = at;
  *num_frames = total;
  return MGX_OK;
}

int mgx_extract_gather_device(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                              const mgx_outputs* o, const mgx_aux_outputs* aux, void* stream) {
  mgx::Outputs x;
  const int rc = make_outputs(p, o, aux, &x);
  if (rc) return rc;
  if (nframes == 0) return MGX_OK;
  if (!starts) return fail(MGX_E_INVALID_ARGUMENT, "starts is NULL");
  if (num_samples < (uint64_t)p->n)
    return fail(MGX_E_INVALID_ARGUMENT, "%llu samples hold no buffer of %d", (unsigned long long)num_samples, p->n);
  const GatherLaunch g{starts, num_samples};
  LaunchOpts opt;
  opt.gather = &g;
  return extract_device_impl(p, samples, nframes, (uint64_t)p->n, &x, stream, opt);
}

}  // extern "C"

namespace {

// A stream's scratch set (mgx_plan::ChainRing), the whole set at once: the scalar windows (kScalWords words
// for each wave of the largest grid), the reference-order MFCC's power-row ring (2 FPW x N/2 floats per wave;
// MGX_FLAG_MFCC_REFERENCE plans) and the tail pool's ticket counter (N >= 2048 plans), zeroed in stream order
// before the first launch. On failure nothing is kept and the next call on the stream tries again.
int add_stream_scratch(mgx_plan* p, void* stream) {
  mgx_plan::ChainRing r{};
  r.stream = stream;
  auto undo = [&r]() {
    if (r.done) (void)hipEventDestroy(r.done);
    if (r.scal) (void)hipFree(r.scal);
    if (r.rows) (void)hipFree(r.rows);
    if (r.pool_ctr) (void)hipFree(r.pool_ctr);
  };
  hipError_t e = hipEventCreateWithFlags(&r.done, hipEventDisableTiming);
  if (e != hipSuccess) { r.done = nullptr; return hip_fail(e, "hipEventCreate(stream scratch)"); }
  e = hipMalloc(reinterpret_cast<void**>(&r.scal), (size_t)p->grid_cap * 4 * mgx::kScalWords * sizeof(uint64_t));
  if (e != hipSuccess) { r.scal = nullptr; undo(); return hip_fail(e, "hipMalloc(scalar windows)"); }
  if (p->chain_groups > 0) {
    const size_t fpw = (size_t)mgx::frames_per_batch(p->n) / 4;
    e = hipMalloc(reinterpret_cast<void**>(&r.rows), (size_t)p->grid_cap * 4 * 2 * fpw * (size_t)p->L * sizeof(float));
    if (e != hipSuccess) { r.rows = nullptr; undo(); return hip_fail(e, "hipMalloc(mel chain rows)"); }
  }
  if (p->n >= 2048) {
    e = hipMalloc(reinterpret_cast<void**>(&r.pool_ctr), sizeof(uint64_t));
    if (e != hipSuccess) r.pool_ctr = nullptr;
    else e = hipMemsetAsync(r.pool_ctr, 0, sizeof(uint64_t), (hipStream_t)stream);
    if (e != hipSuccess) { undo(); return hip_fail(e, "tail pool counter"); }
  }
  p->chain_rings.push_back(r);
  return MGX_OK;
}

// mgx_extract_device and mgx_extract_signal_device (stride: the samples from one frame's start to the next, N
// for dense frames), and with opt.done (the small host path) the launch's completion word; opt.inline_frame
// (the small path's one frame in host memory) goes into the kernel arguments where the kernel takes it
// (mgx::launch_extract); opt.res: the plan's resident launch (resident_request). Any other launch ends the
// plan's resident one first, so the plan's own work never waits behind it or shares the device with it.
int extract_device_impl(mgx_plan* p, const float* frames, uint64_t nframes, uint64_t stride, const mgx::Outputs* o, void* stream,
                        const LaunchOpts& opt) {
  const auto [done, inline_frame, res, gather] = opt;
  if (nframes == 0) return MGX_OK;
  if (!frames) return fail(MGX_E_INVALID_ARGUMENT, "frames is NULL");
  if (int rc = check_outputs(*o)) return rc;  // (the device entry points' check; the host paths come checked)
  if (!res) resident_stop(p);
  mgx::KernelArgs a{};
  a.frames = frames;
  a.num_frames = nframes;
  a.frame_stride = stride;
  a.t = p->t;
  a.out = *o;
  a.sample_rate = p->d.sample_rate;
  a.freq_sum = p->freq_sum;
  a.pow_freq_sum = p->pow_freq_sum;
  a.nyq_bin = p->nyq;
  a.sharp_tail_sum = p->sharp_tail;
  a.rcp_ncoef = 1.0 / (double)p->d.num_mfcc_coeffs;
  a.nfilt = (int)p->d.num_mel_bands;
  a.ncoef = (int)p->d.num_mfcc_coeffs;
  a.scalar_f64 = (int)p->d.scalar_f64;
  a.dct_sequential = (p->d.flags & MGX_FLAG_DCT_SEQUENTIAL) ? 1 : 0;
  a.chain_groups = p->chain_groups;
  a.chain_pair = p->chain_pair;
  bool spec = o->loudness_specific || o->mfcc || o->mel_bands || o->amplitude_spectrum || o->power_spectrum || o->complex_real;
  for (int i = MGX_SPECTRAL_CENTROID; i < MGX_NUM_SCALARS; ++i) spec = spec || o->scalars[i];
  a.need_spectrum = spec;
  a.need_loudness = o->loudness_specific || o->scalars[MGX_LOUDNESS_TOTAL] || o->scalars[MGX_PERCEPTUAL_SPREAD] ||
                    o->scalars[MGX_PERCEPTUAL_SHARPNESS];
  a.need_mel = o->mfcc != nullptr || o->mel_bands != nullptr;
  a.need_dct = o->mfcc != nullptr;
  // moment sums: 2 = S1..S4 and sum log2 a, 1 = S1 only, 0 = none
  a.need_mom = (o->scalars[MGX_SPECTRAL_FLATNESS] || o->scalars[MGX_SPECTRAL_SPREAD] ||
                o->scalars[MGX_SPECTRAL_SKEWNESS] || o->scalars[MGX_SPECTRAL_KURTOSIS]) ? 2
               : (o->scalars[MGX_SPECTRAL_CENTROID] || o->scalars[MGX_SPECTRAL_SLOPE]) ? 1 : 0;
  a.need_prefix = a.need_loudness || o->scalars[MGX_SPECTRAL_ROLLOFF];
  a.need_energy = o->scalars[MGX_RMS] || o->scalars[MGX_ENERGY];
  a.need_zcr = o->scalars[MGX_ZCR] != nullptr;
  bool any_scalar = false;
  for (int i = 0; i < MGX_NUM_SCALARS; ++i) any_scalar = any_scalar || o->scalars[i];
  const uint64_t fb = (uint64_t)mgx::frames_per_batch(p->n);
  const uint64_t nb = (nframes + fb - 1) / fb;
  const int cap = std::max(1, p->grid_cap - (res ? 0 : g_resident_live[dev_slot(p)].load(std::memory_order_relaxed)));
  const int grid = (int)std::min<uint64_t>(nb, (uint64_t)cap);
  a.wg_ranks = grid == p->grid_cap && p->cus > 0 ? p->grid_cap / p->cus : 1;
  // The scalars run once per window of a wave's batches (kernels.hip scalar_pass) when the launch
  // computes a spectrum (VALU-bound there: 0.7-1.9 % faster by N, outputs identical) and its waves
  // get at least 8 batches each on average. A time-only launch is HBM-bound, and the windows' late,
  // per-wave output writes lost it 18 %; with a few batches per wave (C2's 65,536 frames: 3) the
  // one pass at the end of each wave lengthens the launch's tail (+1.6 %). Those, and launches
  // without a scalar output, keep the per-batch form.
  a.scal_defer = a.need_spectrum && any_scalar && nb >= (uint64_t)grid * 8;
  // A batch larger than the MALL is read past the caches: it cannot stay resident between launches, and
  // its lines would evict the ones the launch reads back (the scalar windows); N = 1024 all features
  // -1.2 % per launch, the HBM-bound time-only set -12 % (profiles/r05_prologue_ab.txt, r06_nt_frames.txt).
  // A smaller one keeps plain loads: launches over the same frames then find them in the MALL (C2).
  // A signal launch (stride != N) decides by the samples it touches, ((F - 1) stride + N) floats: the same
  // figure for dense frames. Overlapping frames (stride < N) are read again by the next frames of the batch
  // and the workgroup, and plain loads keep their lines for them: N = 1024 at hop 512 / 256, a 512 / 256 MiB
  // signal, the time-only set 0.136 / 0.119 ms plain against 0.163 / 0.149 ms non-temporal (dense frames
  // 0.178), all features -1.8 / -3.0 % plain against +0.5 / -0.8 % (profiles/signal_hop.txt). So they are read
  // non-temporally only when MGX_NT_MIN_MB is set (the tests and tools/signal_bench.py force either kind).
  const bool overlap = stride < (uint64_t)p->n;
  a.nt_frames = (!overlap || p->nt_forced) && ((nframes - 1) * stride + (uint64_t)p->n) * sizeof(float) > p->nt_min_bytes;
  if (gather) {
    // A gather launch (stride is not read): the table is the kernel's to see, not the host's, so whether its
    // frames overlap is judged by count -- more samples read than there are (nframes N > num_samples) means
    // lines read more than once, which plain loads keep, as for a signal's overlapping frames; otherwise the
    // dense rule on the samples' bytes. MGX_NT_MIN_MB decides for both, as above.
    const bool reread = nframes * (uint64_t)p->n > gather->num_samples;
    a.nt_frames = (!reread || p->nt_forced) && gather->num_samples * sizeof(float) > p->nt_min_bytes;
  }
  hipError_t e = hipSetDevice(p->d.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  if (res) {
    // the resident launch: one frame per request from the mailbox (the frame pointer only feeds the kernel's
    // ignored prefetch: a valid table), no stream scratch (one frame: no windows, no pool, no chains)
    a.frames = p->t.window;
    a.res_mail = p->d_mail;
    a.res_exit = reinterpret_cast<uint32_t*>(p->d_mail + p->n);
    a.res_seq = res->seq;
    a.res_idle = p->res_idle_ms * 100000u;  // the 100 MHz real-time clock
    a.res_light = p->res_light ? 1 : 0;
    a.done_flag = const_cast<uint32_t*>(done);
    e = mgx::launch_extract(p->n, (int)p->d.precision, (int)p->d.mode, a, 1, (hipStream_t)stream, nullptr, true);
    return e == hipSuccess ? MGX_OK : hip_fail(e, "resident launch");
  }
  // the stream's scratch set: allocated whole by the first launch on the stream, whatever its shape, so one
  // untimed call per stream sets the stream up for every later call (include/meyda_gpu.h)
  mgx_plan::ChainRing* ring = nullptr;
  for (auto& r : p->chain_rings)
    if (r.stream == stream) ring = &r;
  if (!ring) {
    int rc = add_stream_scratch(p, stream);
    if (rc) return rc;
    ring = &p->chain_rings.back();
  }
  if (a.scal_defer) a.scal_rows = ring->scal;
  if (a.chain_groups > 0 && a.need_spectrum && a.need_mel) a.chain_rows = ring->rows;
  // The tail pool at N = 2048 (the kernels without a frame prefetch; not the reference-order ones): the
  // last pool_pct percent of the groups taken by ticket (kernels.hip; 15 %: -2.7 % per launch against the static
  // shares alone, outputs identical, profiles/r05_tail_pool.txt). N = 4096, without a prefetch either, takes
  // 2048's setting.
  if (p->n >= 2048 && !(a.chain_groups > 0 && a.need_spectrum && a.need_mel) && p->pool_pct > 0) {
    // (nb here counts groups of 16 frames, the kernel's groups; the pool's tickets are batches of 4 frames)
    const uint64_t ng_all = nb, pg = ng_all * (uint64_t)p->pool_pct / 100;
    if (pg > 0 && pg < ng_all && ring->pool_ctr) {
      a.pool_ctr = ring->pool_ctr;
      a.pool_groups = (uint32_t)pg;
    }
  }
  // (a launch on the plan's own compute stream records no event: destroy synchronises that
  // stream, and the small host path saves the record's ~1 us per call)
  // (a NULL caller stream is never the plan's: s_comp may not exist yet, and then both are NULL)
  hipEvent_t ring_done = (p->s_comp != nullptr && stream == static_cast<void*>(p->s_comp)) ? nullptr : ring->done;
  // (a launch captured into a graph records no event either: the graph's replays are the caller's to
  // wait for before mgx_plan_destroy, as any work it launches on the plan's memory)
  if (ring_done) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) ring_done = nullptr;
  }
  if (done) {
    a.done_flag = const_cast<uint32_t*>(done);
    a.done_count = p->d_done_count;
    a.done_seq = p->done_seq;
    a.done_waves = (uint32_t)grid * 4;
  }
  // (a gather launch: its table beside the arguments, the last start whose frame lies inside the samples)
  const mgx::GatherTable gt{gather ? gather->starts : nullptr, gather ? gather->num_samples - (uint64_t)p->n : 0};
  e = mgx::launch_extract(p->n, (int)p->d.precision, (int)p->d.mode, a, grid, (hipStream_t)stream, inline_frame, false,
                          gather ? &gt : nullptr);
  if (e != hipSuccess) return hip_fail(e, "extract kernel launch");
  if (ring_done) {
    e = hipEventRecord(ring_done, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "hipEventRecord(mel chain rows)");
  }
  return MGX_OK;
}

}  // namespace

namespace {

// Host batches: `nframes` frames through two plan-owned device slots, host_chunk frames at a
// time. `fill(f0, cnt, slot, stream)` enqueues the copy of frames [f0, f0 + cnt) into slot
// `slot` (p->s_frames[slot]) on the copy stream. Chunk i+1's host-to-device copy runs while
// chunk i is extracted on the compute stream; chunk i's outputs then return to the host
// arrays of `o` (laid out over all nframes) on the copy stream.
int ensure_host_staging(mgx_plan* p, uint64_t chunk, size_t out_bytes) {
  hipError_t e = hipSetDevice(p->d.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  if (!p->s_copy) {
    // (the small host path may have created s_comp already: it is created once, never replaced)
    e = hipStreamCreateWithFlags(&p->s_copy, hipStreamNonBlocking);
    if (e == hipSuccess && !p->s_comp) e = hipStreamCreateWithFlags(&p->s_comp, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
      e = hipEventCreateWithFlags(&p->ev_loaded[i], hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev_done[i], hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev_back[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) return hip_fail(e, "host staging streams");
  }
  if (p->s_chunk >= chunk && p->s_out_bytes >= out_bytes) return MGX_OK;
  for (int i = 0; i < 2; ++i) {
    if (p->s_frames[i]) (void)hipFree(p->s_frames[i]);
    if (p->s_out[i]) (void)hipFree(p->s_out[i]);
    p->s_frames[i] = nullptr;
    p->s_out[i] = nullptr;
  }
  p->s_chunk = 0;
  p->s_out_bytes = 0;
  for (int i = 0; i < 2; ++i) {
    e = hipMalloc(reinterpret_cast<void**>(&p->s_frames[i]), chunk * p->n * sizeof(float));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(staging frames)");
    e = hipMalloc(reinterpret_cast<void**>(&p->s_out[i]), out_bytes);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(staging outputs)");
  }
  p->s_chunk = chunk;
  p->s_out_bytes = out_bytes;
  return MGX_OK;
}

// Device bytes per frame of the requested outputs (host staging layouts).
size_t out_bytes_per_frame(const mgx_plan* p, uint32_t fields) {
  size_t per = 0;
  for (int i = 0; i < mgx::kOutFields; ++i) per += (fields >> i) & 1u ? mgx::out_field_bytes(p->d, i) : 0;
  return per;
}

// Ends the plan's resident launch if one may be on the device: the stop word into the mailbox's first word
// (kernels.hip res_take), then its stream (one that already ended on its idle timeout costs only the
// synchronisation).
void resident_ended(mgx_plan* p) {
  p->res_live = false;
  g_resident_live[dev_slot(p)].fetch_sub(1, std::memory_order_relaxed);
}

void resident_stop(mgx_plan* p) {
  if (!p->res_live) return;
  __atomic_store_n(&p->h_mail[0], (uint64_t)mgx::kResStop << 32, __ATOMIC_RELEASE);
  (void)hipStreamSynchronize(p->s_res);
  resident_ended(p);
}

// bit k: field k of mgx_outputs requested. The resident launch serves those fields alone: a request for a
// later one (mel_bands) is served by a launch of its own (extract_host_small), so it is no part of the key.
uint32_t output_key(const mgx::Outputs* o) { return mgx::out_requested(*o) & mgx::kGroupFieldBits; }

// One frame (in p->h_in) through the plan's resident launch (MGX_FLAG_RESIDENT), its outputs landing in the
// small path's pinned layout h (device addresses d) under request number seq:
//  * a live launch that writes another output layout, or waits for another request number (a call of
//    another kind ended it, or the numbers wrapped), is ended first: its kernel arguments fix both;
//  * the frame goes into the mailbox, each word one 8-byte store tagged with seq (kernels.hip res_wait);
//  * a launch that ended on its idle timeout is collected, and one is started when none is live -- after
//    the post, so its first read finds the frame;
//  * the host spins on the completion word, which the launch releases after each request's outputs (a launch
//    that does not end leaves its plain stores in the GPU's L2 until a release writes them back: the output
//    words themselves cannot be waited on as the one-launch path does). A launch that ends while the host
//    waits (it read the mailbox before the frame landed, then timed out) is started again, twice at most;
//    past 1 s the call fails with the launch ended.
int resident_request(mgx_plan* p, const mgx::Outputs* o, const mgx::Outputs& d, uint32_t seq) {
  const int n = p->n;
  hipError_t e = hipSuccess;
  const uint32_t key = output_key(o);
  if (p->res_live && (p->res_key != key || p->res_next != seq)) resident_stop(p);
  if (!p->h_mail) {
    uint64_t* hm = nullptr;
    const size_t bytes = (size_t)(n + 8) * sizeof(uint64_t);  // the words, then a 64-byte line for the exit word
    e = hipHostMalloc(reinterpret_cast<void**>(&hm), bytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(resident mailbox)");
    memset(hm, 0, bytes);
    e = hipHostGetDevicePointer(reinterpret_cast<void**>(&p->d_mail), hm, 0);
    if (e != hipSuccess) {
      (void)hipHostFree(hm);
      return hip_fail(e, "hipHostGetDevicePointer(resident mailbox)");
    }
    p->h_mail = hm;
  }
  if (!p->s_res) {
    // A stream with a CU mask (every CU) gets a hardware queue of its own: the HIP runtime spreads ordinary
    // streams over a few shared queues, and a queue shared with the resident launch would hold every later
    // kernel of the other stream behind it until its idle timeout (tests/test_gpu_resident.py).
    std::vector<uint32_t> mask((size_t)(p->cus + 31) / 32, 0xFFFFFFFFu);
    e = hipExtStreamCreateWithCUMask(&p->s_res, (uint32_t)mask.size(), mask.data());
    if (e != hipSuccess) return hip_fail(e, "hipExtStreamCreateWithCUMask(resident)");
  }
  // (two words per 16-byte store, the samples interleaved with seq: each aligned 8-byte half is written whole,
  // which is all the device's word-by-word check needs. Half the stores of word-by-word writes; the call's
  // time did not move measurably, the device's reads overlap the post.)
  const float* src = p->h_in;
  const __m128i sq = _mm_set1_epi32((int)seq);
  for (int i = 0; i < n; i += 4) {
    const __m128i xv = _mm_castps_si128(_mm_loadu_ps(src + i));
    _mm_store_si128(reinterpret_cast<__m128i*>(p->h_mail + i), _mm_unpacklo_epi32(xv, sq));
    _mm_store_si128(reinterpret_cast<__m128i*>(p->h_mail + i + 2), _mm_unpackhi_epi32(xv, sq));
  }
  std::atomic_thread_fence(std::memory_order_release);
  uint32_t* const exitw = reinterpret_cast<uint32_t*>(p->h_mail + n);
  auto collect = [&]() -> int {  // the launch has ended (its exit word): its stream, for a fault it may report
    e = hipStreamSynchronize(p->s_res);
    resident_ended(p);
    return e == hipSuccess ? MGX_OK : hip_fail(e, "resident launch");
  };
  auto start = [&]() -> int {
    __atomic_store_n(exitw, 0u, __ATOMIC_RELEASE);
    const ResidentLaunch rl{seq};
    LaunchOpts opt;
    opt.done = p->d_done_map;
    opt.res = &rl;
    const int rc = extract_device_impl(p, p->t.window, 1, (uint64_t)p->n, &d, p->s_res, opt);
    if (rc) return rc;
    p->res_live = true;
    g_resident_live[dev_slot(p)].fetch_add(1, std::memory_order_relaxed);
    p->res_key = key;
    return MGX_OK;
  };
  int rc = MGX_OK;
  if (p->res_live && __atomic_load_n(exitw, __ATOMIC_ACQUIRE) != 0) rc = collect();
  if (!rc && !p->res_live) rc = start();
  if (rc) return rc;
  p->res_next = seq + 1;
  auto landed = [&]() { return __atomic_load_n(p->h_done, __ATOMIC_ACQUIRE) == seq; };
  const auto t0 = std::chrono::steady_clock::now();
  int restarts = 0;
  for (unsigned spins = 0;; ++spins) {
    if (landed()) break;
    __builtin_ia32_pause();
    if ((spins & 63) != 63) continue;
    const auto now = std::chrono::steady_clock::now();
    if (__atomic_load_n(exitw, __ATOMIC_ACQUIRE) != 0) {
      if ((rc = collect())) return rc;
      if (landed()) break;
      if (++restarts > 2) return fail(MGX_E_DEVICE, "resident launch: request %u not answered", seq);
      if ((rc = start())) return rc;
      continue;
    }
    if (now - t0 > std::chrono::seconds(1)) {
      resident_stop(p);
      return fail(MGX_E_DEVICE, "resident launch: request %u not answered within 1 s", seq);
    }
  }
  return MGX_OK;
}

// The small path's pinned buffers (mapped into the device, coherent), grown to the call's sizes, and its stream.
int small_buffers(mgx_plan* p, size_t in_bytes, size_t out_bytes) {
  hipError_t e = hipSetDevice(p->d.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  if (!p->s_comp) {
    e = hipStreamCreateWithFlags(&p->s_comp, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
  }
  // (a one-frame call may return before its launch has ended (the output words below): nothing may free
  // or reuse the pinned buffers under it)
  if (p->h_in_bytes < in_bytes || p->h_out_bytes < out_bytes) {
    resident_stop(p);  // (it writes into h_out)
    e = hipStreamSynchronize(p->s_comp);
    if (e != hipSuccess) return hip_fail(e, "small host batch (previous launch)");
  }
  if (p->h_in_bytes < in_bytes) {
    if (p->h_in) (void)hipHostFree(p->h_in);
    p->h_in = nullptr;
    p->h_in_bytes = 0;
    const size_t want = std::max<size_t>(in_bytes, 16 * (size_t)p->n * sizeof(float));
    e = hipHostMalloc(reinterpret_cast<void**>(&p->h_in), want, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(small batch frames)");
    e = hipHostGetDevicePointer(&p->d_in_map, p->h_in, 0);
    if (e != hipSuccess) return hip_fail(e, "hipHostGetDevicePointer(small batch frames)");
    p->h_in_bytes = want;
  }
  if (p->h_out_bytes < out_bytes) {
    if (p->h_out) (void)hipHostFree(p->h_out);
    p->h_out = nullptr;
    p->h_out_bytes = 0;
    e = hipHostMalloc(reinterpret_cast<void**>(&p->h_out), out_bytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(small batch outputs)");
    e = hipHostGetDevicePointer(&p->d_out_map, p->h_out, 0);
    if (e != hipSuccess) return hip_fail(e, "hipHostGetDevicePointer(small batch outputs)");
    p->h_out_bytes = out_bytes;
  }
  return MGX_OK;
}

// The small path's completion word (mgx_plan::h_done) and the device counter behind it, made once.
int small_done_word(mgx_plan* p) {
  if (p->h_done) return MGX_OK;
  uint32_t* hd = nullptr;
  hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&hd), 64, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(completion word)");
  *hd = 0;
  e = hipMalloc(reinterpret_cast<void**>(&p->d_done_count), sizeof(uint32_t));
  // (on the stream the launches run on: a null-stream memset of device memory may return before it has
  // run, and the non-blocking s_comp does not wait for it -- the first launch's waves could count first)
  if (e == hipSuccess) e = hipMemsetAsync(p->d_done_count, 0, sizeof(uint32_t), p->s_comp);
  if (e != hipSuccess) {
    (void)hipHostFree(hd);
    return hip_fail(e, "completion counter");
  }
  e = hipHostGetDevicePointer(reinterpret_cast<void**>(&p->d_done_map), hd, 0);
  if (e != hipSuccess) {
    (void)hipHostFree(hd);
    return hip_fail(e, "hipHostGetDevicePointer(completion word)");
  }
  p->h_done = hd;
  return MGX_OK;
}

// One frame without spectrum outputs (at most 13 + 24 + 32 + 64 words): the host waits on the output words
// themselves -- each preset to an all-ones NaN and polled until the kernel's store has landed -- and the
// launch releases no completion word, which spares the system-scope release (a wait for the outputs'
// write acknowledgements) and the word's own trip back. Stores of 4 and 8 aligned bytes arrive whole: a
// field's words are 8 bytes for an f64 scalar and 4 otherwise. An output that is itself that NaN (a NaN
// input can carry any payload) only ends the spin at its limit.
// Before the launch: the one frame's requested fields (h: their host addresses), all ones.
void preset_output_words(const mgx_plan* p, uint32_t fields, const mgx::Outputs& h) {
  for (int i = 0; i < mgx::kOutFields; ++i)
    if ((fields >> i) & 1u) memset(mgx::out_field(h, i), 0xFF, mgx::out_field_bytes(p->d, i));
  std::atomic_thread_fence(std::memory_order_release);
}

// After it: every word of every requested field in field order, then the stream if the spin ran out.
int wait_output_words(mgx_plan* p, uint32_t fields, const mgx::Outputs& h) {
  constexpr uint64_t kSent = ~(uint64_t)0;
  const auto t0 = std::chrono::steady_clock::now();
  bool late = false;
  unsigned spins = 0;
  auto wait_word = [&](const void* w, size_t bytes) {
    for (;; ++spins) {
      const uint64_t v = bytes == 8 ? __atomic_load_n(static_cast<const uint64_t*>(w), __ATOMIC_ACQUIRE)
                                    : (uint64_t)__atomic_load_n(static_cast<const uint32_t*>(w), __ATOMIC_ACQUIRE);
      if (v != (bytes == 8 ? kSent : (uint64_t)0xFFFFFFFFu)) return;
      __builtin_ia32_pause();
      if (late || ((spins & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(kSmallSpinUs))) {
        late = true;
        return;
      }
    }
  };
  for (int i = 0; i < mgx::kOutFields; ++i) {
    if (!((fields >> i) & 1u)) continue;
    const size_t word = i < MGX_NUM_SCALARS && p->d.scalar_f64 ? 8 : 4, bytes = mgx::out_field_bytes(p->d, i);
    const unsigned char* w = static_cast<const unsigned char*>(mgx::out_field(h, i));
    for (size_t at = 0; at < bytes; at += word) wait_word(w + at, word);
  }
  if (late) {  // a busy device, a failed launch, or an output equal to the preset: the stream decides
    const hipError_t e = hipStreamSynchronize(p->s_comp);
    if (e != hipSuccess) return hip_fail(e, "small host batch");
  }
  return MGX_OK;
}

// The last wave of the launch releases done_seq to the host word after every output store is
// visible (kernels.hip done_signal): polling it returns ~9 us sooner than waiting for the
// stream (tools/ubench/small_latency.hip). Past 20 ms (a busy device) the wait blocks on the
// stream instead, which also reports a failed launch. The spin pauses the core between reads
// (a contended device leaves N-API worker threads waiting here) and gives up after kSmallSpinUs.
int wait_done_word(mgx_plan* p) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n(p->h_done, __ATOMIC_ACQUIRE) == p->done_seq) return MGX_OK;
    __builtin_ia32_pause();
    if ((spins & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(kSmallSpinUs)) break;
  }
  const hipError_t e = hipStreamSynchronize(p->s_comp);
  if (e != hipSuccess) return hip_fail(e, "small host batch");
  if (__atomic_load_n(p->h_done, __ATOMIC_ACQUIRE) != p->done_seq)
    return fail(MGX_E_DEVICE, "small host batch: the launch completed without its completion word");
  return MGX_OK;
}

// A small host batch (at most p->small_max frames): the frames into the plan's pinned input
// buffer, one launch that reads them over PCIe and writes the features into the pinned output
// buffer, one synchronisation, the features out to the caller's arrays. `fill(dst)` writes the
// batch's float32 frames to host memory at dst. The buffers are coherent (fine-grained) host
// memory mapped into the device, so no cache of either side holds a stale copy between calls.
// stride: the samples from one frame's start to the next in what `fill` writes, (nframes - 1) stride + N
// samples in all (N: dense frames; a signal's hop <= N: its samples as they are, each written once).
template <typename Fill>
int extract_host_small(mgx_plan* p, uint64_t nframes, uint64_t stride, const mgx::Outputs* o, Fill fill) {
  const uint32_t fields = mgx::out_requested(*o);
  const size_t in_bytes = ((nframes - 1) * (size_t)stride + (size_t)p->n) * sizeof(float);
  const size_t out_bytes = out_bytes_per_frame(p, fields) * nframes + mgx::kOutLayoutSlack;
  int rc = small_buffers(p, in_bytes, out_bytes);
  if (rc) return rc;
  rc = fill(p->h_in);
  if (rc) return rc;
  // one layout, the device's addresses (d) and the host's (h)
  uint64_t off[mgx::kOutFields];
  mgx::out_layout(p->d, fields, nframes, off);
  const mgx::Outputs d = mgx::out_at(static_cast<unsigned char*>(p->d_out_map), off);
  const mgx::Outputs h = mgx::out_at(p->h_out, off);
  rc = small_done_word(p);
  if (rc) return rc;
  // never 0 (the word's initial value) nor the resident launch's stop word
  p->done_seq = (p->done_seq + 1 == 0 || p->done_seq + 1 == mgx::kResStop) ? 1 : p->done_seq + 1;
  const bool word_wait = nframes == 1 && !(fields & mgx::kSpectrumFieldBits);  // (wait_output_words)
  // MGX_FLAG_RESIDENT: the resident workgroup serves one-frame calls for the mgx_outputs fields; one that asks
  // for a later field (mel_bands) takes the launch below (which ends the resident one first, as any other launch does)
  const bool res = p->resident && nframes == 1 && !(fields & ~mgx::kGroupFieldBits);
  if (res) {
    rc = resident_request(p, o, d, p->done_seq);
    if (rc) return rc;
  } else {
    if (word_wait) preset_output_words(p, fields, h);
    // (one frame: also handed over in the kernel arguments, read there by the kernels that take it)
    LaunchOpts opt;
    opt.done = word_wait ? nullptr : p->d_done_map;
    opt.inline_frame = nframes == 1 ? p->h_in : nullptr;
    rc = extract_device_impl(p, static_cast<const float*>(p->d_in_map), nframes, stride, &d, p->s_comp, opt);
    if (rc) {
      (void)hipStreamSynchronize(p->s_comp);
      return rc;
    }
    rc = word_wait ? wait_output_words(p, fields, h) : wait_done_word(p);
    if (rc) return rc;
  }
  for (int i = 0; i < mgx::kOutFields; ++i)
    if ((fields >> i) & 1u) memcpy(mgx::out_field(*o, i), mgx::out_field(h, i), nframes * mgx::out_field_bytes(p->d, i));
  return MGX_OK;
}

// Dense frames per chunk: kHostChunk while kHostChunk N floats fit a slot (N <= 2048), then as many as do.
uint64_t host_chunk(const mgx_plan* p) { return std::min<uint64_t>(kHostChunk, kHostSlotFloats / (uint64_t)p->n); }

// The frames of a chunk, for a signal cut at `hop` (signal_chunk_frames(p, n) = host_chunk(p) for dense
// frames): a chunk of K frames occupies (K - 1) hop + N floats of its slot, and a slot holds host_chunk N,
// so up to hop = N a chunk keeps its host_chunk frames, and a larger hop (samples skipped) gets as many
// frames as still fit, one at least.
uint64_t signal_chunk_frames(const mgx_plan* p, uint64_t hop) {
  const uint64_t n = (uint64_t)p->n, hc = host_chunk(p);
  return hop <= n ? hc : std::max<uint64_t>(1, (hc * n - n) / hop + 1);
}

// The chunks of a gather call (mgx_extract_gather_host): chunk i is frames [bounds[i], bounds[i + 1]), whose
// samples are the span [lo[i], lo[i] + span[i]) of the caller's array; `fill` copies that span into the slot and
// the chunk's starts, less lo[i], into p->s_starts[slot].
struct GatherChunks {
  std::vector<uint64_t> bounds, lo, span;
};

// stride: the samples between the starts of consecutive frames in a slot (N: dense frames; a signal's
// hop: `fill` then writes a chunk's (cnt - 1) stride + N samples); chunk_max: frames per chunk.
// gc: the chunks are gc's instead (chunk_max: the longest of them), each launched over its slot's table of starts.
// hook (mgx_summarize_host): its `pooled` fields are computed and laid out in the slot beside the ones the caller
// named, but do not cross back; after(f0, cnt, d) enqueues the chunk's reduction on the compute stream, over the
// chunk's records where they lie (d). Without a hook nothing here differs from what it was.
struct ChunkHook {
  uint32_t pooled;
  std::function<int(uint64_t f0, uint64_t cnt, const mgx::Outputs& d)> after;
};

template <typename Fill>
int extract_host_chunked(mgx_plan* p, uint64_t nframes, uint64_t stride, uint64_t chunk_max, const mgx::Outputs* o, Fill fill,
                         const GatherChunks* gc = nullptr, const ChunkHook* hook = nullptr) {
  const int n = p->n;
  const uint32_t back = mgx::out_requested(*o);  // the fields that return to the caller's arrays
  const uint32_t fields = back | (hook ? hook->pooled : 0u);
  // device bytes per frame for the requested outputs
  const size_t per = out_bytes_per_frame(p, fields);
  const uint64_t chunk = std::min<uint64_t>(nframes, chunk_max);
  // (the slot in whole frames of N floats: the chunk's span, at most kHostChunk frames' worth)
  uint64_t slot_frames = ((chunk - 1) * stride + (uint64_t)n + (uint64_t)n - 1) / (uint64_t)n;
  if (gc) slot_frames = (*std::max_element(gc->span.begin(), gc->span.end()) + (uint64_t)n - 1) / (uint64_t)n;
  int rc = ensure_host_staging(p, slot_frames, per * chunk + mgx::kOutLayoutSlack);
  if (rc) return rc;
  const uint64_t nch = gc ? gc->lo.size() : (nframes + chunk - 1) / chunk;
  // chunk i's first frame and count
  auto first = [&](uint64_t i) { return gc ? gc->bounds[i] : i * chunk; };
  auto count = [&](uint64_t i) { return gc ? gc->bounds[i + 1] - gc->bounds[i] : std::min<uint64_t>(chunk, nframes - i * chunk); };
  hipError_t e = hipSuccess;
  auto fail_sync = [&](int code) {  // leave no work in flight on the plan's buffers
    (void)hipStreamSynchronize(p->s_comp);
    (void)hipStreamSynchronize(p->s_copy);
    return code;
  };
  rc = fill(0, count(0), 0, p->s_copy);
  if (rc) return fail_sync(rc);
  e = hipEventRecord(p->ev_loaded[0], p->s_copy);
  for (uint64_t i = 0; i < nch && e == hipSuccess; ++i) {
    const int sl = (int)(i & 1);
    const uint64_t f0 = first(i), cnt = count(i);
    uint64_t off[mgx::kOutFields];
    mgx::out_layout(p->d, fields, cnt, off);
    const mgx::Outputs d = mgx::out_at(p->s_out[sl], off);
    // extraction of chunk i: after its frames arrived and chunk i-2's outputs left the slot
    e = hipStreamWaitEvent(p->s_comp, p->ev_loaded[sl], 0);
    if (e == hipSuccess && i >= 2) e = hipStreamWaitEvent(p->s_comp, p->ev_back[sl], 0);
    if (e != hipSuccess) break;
    const GatherLaunch g{p->s_starts[sl], gc ? gc->span[i] : 0};
    LaunchOpts opt;
    opt.gather = gc ? &g : nullptr;
    rc = extract_device_impl(p, p->s_frames[sl], cnt, stride, &d, p->s_comp, opt);
    if (rc) return fail_sync(rc);
    if (hook && (rc = hook->after(f0, cnt, d))) return fail_sync(rc);
    e = hipEventRecord(p->ev_done[sl], p->s_comp);
    // chunk i+1's frames into the other slot once chunk i-1's extraction has read them
    if (e == hipSuccess && i + 1 < nch) {
      if (i >= 1) e = hipStreamWaitEvent(p->s_copy, p->ev_done[sl ^ 1], 0);
      if (e != hipSuccess) break;
      rc = fill(first(i + 1), count(i + 1), sl ^ 1, p->s_copy);
      if (rc) return fail_sync(rc);
      e = hipEventRecord(p->ev_loaded[sl ^ 1], p->s_copy);
    }
    // chunk i's outputs back to the caller's arrays
    if (e == hipSuccess) e = hipStreamWaitEvent(p->s_copy, p->ev_done[sl], 0);
    for (int k = 0; k < mgx::kOutFields && e == hipSuccess; ++k) {
      if (!((back >> k) & 1u)) continue;
      const uint64_t fb = mgx::out_field_bytes(p->d, k);
      e = hipMemcpyAsync(static_cast<unsigned char*>(mgx::out_field(*o, k)) + f0 * fb, mgx::out_field(d, k), cnt * fb,
                         hipMemcpyDeviceToHost, p->s_copy);
    }
    if (e == hipSuccess) e = hipEventRecord(p->ev_back[sl], p->s_copy);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(p->s_copy);
  if (e != hipSuccess) return fail_sync(hip_fail(e, "host batch copies"));
  return MGX_OK;
}

uint32_t sample_bytes(uint32_t format) {
  switch (format) {
    case MGX_PCM_F32: return 4;
    case MGX_PCM_S16: return 2;
    case MGX_PCM_U8: return 1;
    case MGX_PCM_S24: return 3;
    case MGX_PCM_S32: return 4;
    default: return 0;
  }
}

uint16_t rd16(const unsigned char* b) { return (uint16_t)(b[0] | (b[1] << 8)); }
uint32_t rd32(const unsigned char* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }

// The chunked path of mgx_extract_gather_host (starts checked by the caller; hook: extract_host_chunked).
int gather_host_chunked(mgx_plan* p, const float* samples, const uint64_t* starts, uint64_t nframes, const mgx::Outputs* o,
                        const ChunkHook* hook) {
  // Chunks: the longest runs of consecutive buffers of at most host_chunk whose span, max start + N - min start,
  // fits a slot of the dense path (host_chunk N floats; one buffer always does). Sorted starts no further apart
  // than N fill their chunks; any other order is served, in as many chunks as its jumps make.
  GatherChunks gc;
  std::vector<uint64_t> rel(nframes);  // every start less its chunk's lowest: what the chunk's launch reads
  const uint64_t n = (uint64_t)p->n, hc = host_chunk(p), slot = hc * n;
  uint64_t longest = 0;
  for (uint64_t f0 = 0; f0 < nframes;) {
    uint64_t lo = starts[f0], hi = starts[f0], f1 = f0 + 1;
    for (; f1 < nframes && f1 - f0 < hc; ++f1) {
      const uint64_t l = std::min(lo, starts[f1]), h = std::max(hi, starts[f1]);
      if (h - l + n > slot) break;
      lo = l;
      hi = h;
    }
    for (uint64_t f = f0; f < f1; ++f) rel[f] = starts[f] - lo;
    gc.bounds.push_back(f0);
    gc.lo.push_back(lo);
    gc.span.push_back(hi - lo + n);
    longest = std::max(longest, f1 - f0);
    f0 = f1;
  }
  gc.bounds.push_back(nframes);
  if (!p->s_starts[0]) {
    hipError_t e = hipSetDevice(p->d.device);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
      e = hipMalloc(reinterpret_cast<void**>(&p->s_starts[i]), kHostChunk * sizeof(uint64_t));
      if (e != hipSuccess) p->s_starts[i] = nullptr;
    }
    if (e != hipSuccess) {
      if (p->s_starts[0]) (void)hipFree(p->s_starts[0]);
      p->s_starts[0] = nullptr;
      return hip_fail(e, "hipMalloc(staging starts)");
    }
  }
  uint64_t ci = 0;  // (fill is called for the chunks in order, once each)
  return extract_host_chunked(p, nframes, n, longest, o, [&](uint64_t f0, uint64_t cnt, int sl, hipStream_t st) {
    const uint64_t i = ci++;
    hipError_t e = hipMemcpyAsync(p->s_frames[sl], samples + gc.lo[i], gc.span[i] * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(p->s_starts[sl], rel.data() + f0, cnt * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    return e == hipSuccess ? MGX_OK : hip_fail(e, "hipMemcpyAsync(samples, starts)");
  }, &gc, hook);
}

}  // namespace

extern "C" {

int mgx_extract_host(mgx_plan* p, const float* frames, uint64_t nframes, const mgx_outputs* o) {
  if (!p || !o) return fail(MGX_E_INVALID_ARGUMENT, "NULL plan or outputs");
  return mgx_extract_host_ex(p, frames, nframes * (uint64_t)p->n, (uint32_t)p->n, o, nullptr);
}

int mgx_extract_signal_host(mgx_plan* p, const float* samples, uint64_t num_samples, uint32_t hop, const mgx_outputs* o) {
  return mgx_extract_host_ex(p, samples, num_samples, hop, o, nullptr);
}

int mgx_extract_host_ex(mgx_plan* p, const float* samples, uint64_t num_samples, uint32_t hop, const mgx_outputs* outputs,
                        const mgx_aux_outputs* aux) {
  mgx::Outputs x;
  int rc = make_outputs(p, outputs, aux, &x);
  if (rc) return rc;
  const mgx::Outputs* const o = &x;
  uint64_t nframes = 0;
  rc = mgx_signal_frames(num_samples, (uint32_t)p->n, hop, &nframes);
  if (rc) return rc;
  if (nframes == 0) return MGX_OK;
  if (!samples) return fail(MGX_E_INVALID_ARGUMENT, "samples is NULL");
  if ((rc = check_outputs(x))) return rc;
  const int n = p->n;
  const uint64_t h = hop;
  if (nframes <= p->small_max) {
    // up to hop = N the samples as they are (each written to the pinned buffer once, read at stride hop);
    // a larger hop gathers its frames densely, so the buffer never exceeds the dense path's
    if (h <= (uint64_t)n)
      return extract_host_small(p, nframes, h, o, [&](float* dst) {
        memcpy(dst, samples, ((nframes - 1) * h + (size_t)n) * sizeof(float));
        return MGX_OK;
      });
    return extract_host_small(p, nframes, (uint64_t)n, o, [&](float* dst) {
      for (uint64_t f = 0; f < nframes; ++f) memcpy(dst + f * n, samples + f * h, (size_t)n * sizeof(float));
      return MGX_OK;
    });
  }
  return extract_host_chunked(p, nframes, h, signal_chunk_frames(p, h), o, [&](uint64_t f0, uint64_t cnt, int slot, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(p->s_frames[slot], samples + f0 * h, ((cnt - 1) * h + (uint64_t)n) * sizeof(float),
                                  hipMemcpyHostToDevice, st);
    return e == hipSuccess ? MGX_OK : hip_fail(e, "hipMemcpyAsync(samples)");
  });
}

int mgx_extract_gather_host(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                            const mgx_outputs* outputs, const mgx_aux_outputs* aux) {
  mgx::Outputs x;
  int rc = make_outputs(p, outputs, aux, &x);
  if (rc) return rc;
  const mgx::Outputs* const o = &x;
  if (nframes == 0) return MGX_OK;
  if (!starts) return fail(MGX_E_INVALID_ARGUMENT, "starts is NULL");
  if (!samples) return fail(MGX_E_INVALID_ARGUMENT, "samples is NULL");
  const uint64_t n = (uint64_t)p->n;
  if (num_samples < n) return fail(MGX_E_INVALID_ARGUMENT, "%llu samples hold no buffer of %d", (unsigned long long)num_samples, p->n);
  if ((rc = check_outputs(x))) return rc;
  // (the host sees the table: a start whose buffer leaves the samples is refused here, before any copy)
  for (uint64_t f = 0; f < nframes; ++f)
    if (starts[f] > num_samples - n)
      return fail(MGX_E_INVALID_ARGUMENT, "starts[%llu] = %llu: a buffer of %d leaves the %llu samples", (unsigned long long)f,
                  (unsigned long long)starts[f], p->n, (unsigned long long)num_samples);
  // a batch of the one-launch path gathers its buffers densely into the pinned input buffer, as a signal
  // at hop > N does: one buffer then takes the inline-frame launch or the resident workgroup
  if (nframes <= p->small_max)
    return extract_host_small(p, nframes, n, o, [&](float* dst) {
      for (uint64_t f = 0; f < nframes; ++f) memcpy(dst + f * n, samples + starts[f], (size_t)n * sizeof(float));
      return MGX_OK;
    });
  return gather_host_chunked(p, samples, starts, nframes, o, nullptr);
}

}  // extern "C"

namespace {

// mgx_summarize_*: the caller's summary struct as the kernels' list of fields (each with its destination, its
// width and its first column; the sources are set per launch), and the pooled fields as bits of the table of
// output fields (out_fields.h).
struct SummaryFields {
  mgx::SummaryArgs a{};
  int index[mgx::kSummaryFields];  // field i of a.f in the numbering of mgx::out_field
  uint32_t pooled = 0;
};

// The summary struct itself: there, and of exactly this build's size (the check that lets it grow). What every
// summary entry point begins with, ahead of the plan.
int check_summary(const mgx_summary_outputs* s) {
  if (!s) return fail(MGX_E_INVALID_ARGUMENT, "summary is NULL");
  if (s->struct_size != sizeof(mgx_summary_outputs))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_summary_outputs.struct_size is %u, expected %zu", s->struct_size,
                sizeof(mgx_summary_outputs));
  if (s->reserved != 0) return fail(MGX_E_INVALID_ARGUMENT, "mgx_summary_outputs.reserved is %u, expected 0", s->reserved);
  return MGX_OK;
}

void summary_fields(const mgx_plan* p, const mgx_summary_outputs* s, SummaryFields* sf) {
  // (the summary's arrays in the table's numbering: the scalars, then loudness_specific 13, mfcc 14, the
  // amplitude and power spectra 15 and 16, mel_bands 19)
  double* const arrays[] = {s->loudness_specific, s->mfcc, s->amplitude_spectrum, s->power_spectrum, s->mel_bands};
  const int array_index[] = {13, 14, 15, 16, 19};
  static_assert(MGX_NUM_SCALARS + sizeof arrays / sizeof *arrays == mgx::kSummaryFields, "one entry per summary field");
  uint32_t col = 0, nf = 0;
  for (int i = 0; i < mgx::kSummaryFields; ++i) {
    double* const dst = i < MGX_NUM_SCALARS ? s->scalars[i] : arrays[i - MGX_NUM_SCALARS];
    if (!dst) continue;
    const int idx = i < MGX_NUM_SCALARS ? i : array_index[i - MGX_NUM_SCALARS];
    mgx::SummaryField& f = sf->a.f[nf];
    f.dst = dst;
    f.width = idx < MGX_NUM_SCALARS ? 1u : (uint32_t)(mgx::out_field_bytes(p->d, idx) / 4);
    f.col0 = col;
    f.f64 = idx < MGX_NUM_SCALARS && p->d.scalar_f64;
    col += f.width;
    sf->index[nf++] = idx;
    sf->pooled |= 1u << idx;
  }
  sf->a.nfields = nf;
  sf->a.cols = col;
}

// The buffer a summary call works in. The device call's (the caller's workspace): the per-frame arrays of the
// fields `extra` (pooled, not requested per frame), then the table as the kernels read it, the signals' shifts
// and the block partials. The host call's (mgx_plan::s_sum): no per-frame arrays (the staging slots hold them),
// and the summaries themselves at the end. Everything 256-byte aligned; total: a multiple of 256.
struct SummaryLayout {
  uint64_t frames[mgx::kOutFields];
  uint64_t table, shift, part, result, total;
};

// deltas (mgx_summarize_deltas_device): the arrays and the table are kept for the delta rows even when no field is pooled.
SummaryLayout summary_layout(const mgx_plan_desc& d, uint32_t extra, uint32_t cols, uint64_t nframes, uint64_t nsignals, bool result,
                             bool deltas = false) {
  SummaryLayout l{};
  auto take = [&l](uint64_t bytes) {
    const uint64_t at = l.total;
    l.total += (bytes + 255) / 256 * 256;
    return at;
  };
  if ((cols == 0 && !deltas) || nsignals == 0 || nframes == 0) return l;
  take(mgx::out_layout(d, extra, nframes, l.frames));
  l.table = take((nsignals + 1) * sizeof(uint64_t));
  l.shift = take(nsignals * cols * sizeof(double));
  l.part = take((nframes / mgx::kSummaryBlock + nsignals + 1) * mgx::kSummaryWords * cols * sizeof(double));
  if (result) l.result = take(nsignals * MGX_NUM_STATS * cols * sizeof(double));
  return l;
}

// The checks both summary calls share with the gather calls, in their order
int summary_inputs(const mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                   const uint64_t* frame_offsets, uint64_t nsignals) {
  if (nsignals > 0 && !frame_offsets) return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets is NULL");
  if (nframes == 0) return MGX_OK;
  if (!starts) return fail(MGX_E_INVALID_ARGUMENT, "starts is NULL");
  if (!samples) return fail(MGX_E_INVALID_ARGUMENT, "samples is NULL");
  if (num_samples < (uint64_t)p->n)
    return fail(MGX_E_INVALID_ARGUMENT, "%llu samples hold no buffer of %d", (unsigned long long)num_samples, p->n);
  return MGX_OK;
}

// mgx_summarize_deltas_*: the caller's mgx_delta_summaries as two lists of summary fields (k = 0: the delta
// rows', 1: the second-order rows'; destinations the caller's arrays), and the fields whose rows of each order
// the call has to hold: the second order is the delta of the first, so rows[0] has every field either names.
struct DeltaReq {
  uint32_t width = 0;
  SummaryFields sf[2];
  uint32_t rows[2] = {0, 0};
  bool any() const { return rows[0] != 0; }
};

int delta_request(const mgx_plan* p, const mgx_delta_summaries* ds, DeltaReq* q) {
  if (!ds) return MGX_OK;
  if (ds->struct_size != sizeof(mgx_delta_summaries))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_delta_summaries.struct_size is %u, expected %zu", ds->struct_size,
                sizeof(mgx_delta_summaries));
  if (ds->width < 1 || ds->width > MGX_DELTA_MAX_WIDTH)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_delta_summaries.width is %u, expected 1..%d", ds->width, MGX_DELTA_MAX_WIDTH);
  q->width = ds->width;
  const mgx_summary_outputs* const so[2] = {ds->delta, ds->delta2};
  for (int k = 0; k < 2; ++k) {
    if (!so[k]) continue;
    const int rc = check_summary(so[k]);
    if (rc) return rc;
    if (so[k]->amplitude_spectrum || so[k]->power_spectrum)
      return fail(MGX_E_UNSUPPORTED, "deltas of a spectrum are not pooled (mgx_delta_summaries.%s): mgx_delta_device takes its rows",
                  k ? "delta2" : "delta");
    if (p) summary_fields(p, so[k], &q->sf[k]);  // (the checks above come ahead of the plan's own, as check_summary does)
  }
  q->rows[1] = q->sf[1].pooled;
  q->rows[0] = q->sf[0].pooled | q->sf[1].pooled;
  return MGX_OK;
}

// What the deltas add to the buffer a summary call works in, from `base` bytes on: the delta rows of the fields
// q.rows[0] and the second-order rows of q.rows[1] (each laid out as mgx::out_layout lays per-frame arrays out),
// a table of their own when the buffer holds none (the host call's), and per order the shifts, the partials and
// (host call) the summaries. Everything 256-byte aligned; total: base when there is nothing to keep.
struct DeltaLayout {
  uint64_t rows[2][mgx::kOutFields];
  uint64_t table, shift[2], part[2], result[2], total;
};

DeltaLayout delta_layout(const mgx_plan_desc& d, const DeltaReq& q, uint64_t nframes, uint64_t nsignals, bool host, uint64_t base) {
  DeltaLayout l{};
  l.total = base;
  auto take = [&l](uint64_t bytes) {
    const uint64_t at = l.total;
    l.total += (bytes + 255) / 256 * 256;
    return at;
  };
  if (!q.any() || nsignals == 0 || nframes == 0) return l;
  for (int k = 0; k < 2; ++k) {
    const uint64_t at = l.total;
    take(mgx::out_layout(d, q.rows[k], nframes, l.rows[k]));
    for (int i = 0; i < mgx::kOutFields; ++i)
      if (l.rows[k][i] != UINT64_MAX) l.rows[k][i] += at;
  }
  if (host) l.table = take((nsignals + 1) * sizeof(uint64_t));
  for (int k = 0; k < 2; ++k) {
    const uint64_t cols = q.sf[k].a.cols;
    l.shift[k] = take(nsignals * cols * sizeof(double));
    l.part[k] = take((nframes / mgx::kSummaryBlock + nsignals + 1) * mgx::kSummaryWords * cols * sizeof(double));
    if (host) l.result[k] = take(nsignals * MGX_NUM_STATS * cols * sizeof(double));
  }
  return l;
}

// The operator and the pooling of a deltas call, on `st`: x holds the rows of every field of q.rows[0] (nframes
// of them), buf the arrays of `l`, table the num_signals + 1 offsets as the summary kernels read them (device
// memory). Per field the delta rows, then (q.rows[1]) their delta: two passes, the second over the stored rows;
// then the summary kernels over each order's rows into the destinations of q.sf[k] (device pointers here).
int delta_pool(const mgx_plan_desc& d, DeltaReq& q, const mgx::Outputs& x, unsigned char* buf, const DeltaLayout& l,
               const uint64_t* table, uint64_t nframes, uint64_t nsignals, hipStream_t st) {
  hipError_t e = hipSuccess;
  for (int i = 0; i < mgx::kOutFields && e == hipSuccess; ++i) {
    if (!((q.rows[0] >> i) & 1u)) continue;
    const bool f64 = i < MGX_NUM_SCALARS && d.scalar_f64;
    const uint32_t cols = (uint32_t)(mgx::out_field_bytes(d, i) / (f64 ? 8 : 4));
    e = mgx::launch_delta(mgx::out_field(x, i), buf + l.rows[0][i], nframes, cols, f64, table, nsignals, q.width, false, st);
    if (e == hipSuccess && ((q.rows[1] >> i) & 1u))
      e = mgx::launch_delta(buf + l.rows[0][i], buf + l.rows[1][i], nframes, cols, f64, table, nsignals, q.width, false, st);
  }
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    mgx::SummaryArgs& a = q.sf[k].a;
    if (a.cols == 0) continue;
    for (uint32_t i = 0; i < a.nfields; ++i) a.f[i].src = buf + l.rows[k][q.sf[k].index[i]];
    a.num_signals = nsignals;
    a.num_frames = nframes;
    a.table = table;
    a.shift = reinterpret_cast<double*>(buf + l.shift[k]);
    a.part = reinterpret_cast<double*>(buf + l.part[k]);
    a.row0 = 0;
    a.rows = nframes;
    a.slot0 = 0;
    a.nslots = nframes / mgx::kSummaryBlock + nsignals;
    e = mgx::launch_summary_partial(a, st);
    if (e == hipSuccess) e = mgx::launch_summary_final(a, st);
  }
  return e == hipSuccess ? (int)MGX_OK : hip_fail(e, "delta and summary kernel launch");
}

// mgx_onsets_host: the picker behind the host flux call, over the column of its first request
struct PeakHost {
  const mgx_peak_params* params;
  uint64_t* peak_offsets;  // host, num_signals + 1
  uint64_t* peaks;         // host, capacity entries, or null
  uint64_t capacity;
};

int check_peak_params(const mgx_peak_params* pp) {
  if (!pp) return fail(MGX_E_INVALID_ARGUMENT, "params is NULL");
  if (pp->struct_size != sizeof(mgx_peak_params))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_params.struct_size is %u, expected %zu", pp->struct_size, sizeof(mgx_peak_params));
  const uint32_t reach[4] = {pp->pre_max, pp->post_max, pp->pre_avg, pp->post_avg};
  static const char* const name[4] = {"pre_max", "post_max", "pre_avg", "post_avg"};
  for (int i = 0; i < 4; ++i)
    if (reach[i] > MGX_PEAK_MAX_REACH)
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_params.%s is %u, expected 0..%d", name[i], reach[i], MGX_PEAK_MAX_REACH);
  if (pp->delta != pp->delta) return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_params.delta is NaN");
  return MGX_OK;
}

// mgx_beats_host: the tracker behind mgx_tempo_host's route, over the same column, the lags as its periods
struct BeatHost {
  const mgx_beat_params* params;
  const float* gauss;      // host, mgx_beat_tables of params->max_period
  const double* penalty;   // host
  uint64_t* peak_offsets;  // host, num_signals + 1
  uint64_t* peaks;         // host, capacity entries, or null
  uint64_t capacity;
};

int check_beat_params(const mgx_beat_params* bp) {
  if (!bp) return fail(MGX_E_INVALID_ARGUMENT, "params is NULL");
  if (bp->struct_size != sizeof(mgx_beat_params))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_beat_params.struct_size is %u, expected %zu", bp->struct_size, sizeof(mgx_beat_params));
  if (bp->max_period < 1 || bp->max_period > MGX_BEAT_MAX_PERIOD)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_beat_params.max_period is %u, expected 1..%d", bp->max_period, MGX_BEAT_MAX_PERIOD);
  if (bp->trim > 1) return fail(MGX_E_INVALID_ARGUMENT, "mgx_beat_params.trim is %u, expected 0 or 1", bp->trim);
  return MGX_OK;
}

uint64_t beat_gauss_count(uint32_t P) { return ((uint64_t)P + 1) * ((uint64_t)P + 2) / 2; }
uint64_t beat_penalty_count(uint32_t P) { return ((uint64_t)P + 1) * ((uint64_t)P + 1); }

// mgx_tempo_host: the tempogram, its pooling and the pick behind the host flux call, over the column of its request
struct TempoHost {
  const mgx_tempo_params* params;
  const float* window;  // host, W
  const double* prior;  // host, L, or null without lag
  double* summary;      // host, num_signals x MGX_NUM_STATS x L, or null
  uint32_t* lag;        // host, num_signals, or null
  const BeatHost* beats;  // mgx_beats_host: the lags are picked (prior is set) whether `lag` is or not
};

int check_tempo_params(const mgx_tempo_params* tp) {
  if (!tp) return fail(MGX_E_INVALID_ARGUMENT, "params is NULL");
  if (tp->struct_size != sizeof(mgx_tempo_params))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_tempo_params.struct_size is %u, expected %zu", tp->struct_size, sizeof(mgx_tempo_params));
  if (tp->win_length < 2 || tp->win_length > MGX_TEMPOGRAM_MAX_WIN)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_tempo_params.win_length is %u, expected 2..%d", tp->win_length, MGX_TEMPOGRAM_MAX_WIN);
  if (tp->num_lags < 1 || tp->num_lags > tp->win_length)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_tempo_params.num_lags is %u, expected 1..%u (win_length)", tp->num_lags, tp->win_length);
  if (tp->norm >= MGX_NUM_TEMPOGRAM_NORMS)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_tempo_params.norm is %u, expected 0..%d", tp->norm, MGX_NUM_TEMPOGRAM_NORMS - 1);
  if (!(std::isfinite(tp->gain) && tp->gain >= 0)) return fail(MGX_E_INVALID_ARGUMENT, "mgx_tempo_params.gain must be finite and not negative");
  return MGX_OK;
}

// The workspace of mgx_tempo_device: the table, the shifts, the partials, the summaries and, without a tempogram
// output, a pass of rows. S: the signals as the kernels count them (1 without a table).
struct TempoLayout {
  uint64_t table, shift, part, result, rows, total;
};

TempoLayout tempo_layout(uint64_t nframes, uint64_t S, uint32_t L, bool keep_rows) {
  TempoLayout l{};
  uint64_t total = 0;
  auto take = [&total](uint64_t bytes) {
    const uint64_t at = total;
    total += (bytes + 255) / 256 * 256;
    return at;
  };
  l.table = take((S + 1) * sizeof(uint64_t));
  l.shift = take(S * L * sizeof(double));
  l.part = take((nframes / mgx::kSummaryBlock + S + 1) * mgx::kSummaryWords * L * sizeof(double));
  l.result = take(S * MGX_NUM_STATS * L * sizeof(double));
  l.rows = take(keep_rows ? 0 : std::min(nframes, mgx::kTempoChunkRows) * L * sizeof(float));
  l.total = total;
  return l;
}

// mgx_tempo_device after its checks, and the last step of mgx_tempo_host: every pointer a device pointer, S >= 1.
// pool: the rows are pooled, into `summary` or, when that is null, into the workspace's own summaries
hipError_t tempo_run(const void* env, uint64_t nframes, bool f64, const uint64_t* raw_table, uint64_t S, const mgx_tempo_params& tp,
                     const float* window, const double* prior, float* tempogram, double* summary, bool pool, uint32_t* lag,
                     unsigned char* ws, hipStream_t stream) {
  const uint32_t W = tp.win_length, L = tp.num_lags;
  const TempoLayout l = tempo_layout(nframes, S, L, tempogram != nullptr);
  uint64_t* const table = reinterpret_cast<uint64_t*>(ws + l.table);
  hipError_t e = hipSuccess;
  if (nframes > 0)
    e = raw_table ? mgx::launch_summary_table(raw_table, table, S, nframes, stream) : mgx::launch_tempo_one_signal(table, nframes, stream);
  if (!pool) {
    if (e == hipSuccess) e = mgx::launch_tempogram(env, nframes, f64, table, S, window, W, L, tp.norm, tempogram, 0, nframes, stream);
    return e;
  }
  mgx::SummaryArgs a{};
  a.nfields = 1;
  a.cols = L;
  a.f[0].dst = summary ? summary : reinterpret_cast<double*>(ws + l.result);
  a.f[0].width = L;
  a.table = table;
  a.num_signals = S;
  a.num_frames = nframes;
  a.nslots = nframes / mgx::kSummaryBlock + S;
  a.shift = reinterpret_cast<double*>(ws + l.shift);
  a.part = reinterpret_cast<double*>(ws + l.part);
  if (tempogram) {
    if (e == hipSuccess) e = mgx::launch_tempogram(env, nframes, f64, table, S, window, W, L, tp.norm, tempogram, 0, nframes, stream);
    a.f[0].src = tempogram;
    a.rows = nframes;
    if (e == hipSuccess) e = mgx::launch_summary_partial(a, stream);
  } else {
    // a pass of rows at a time through the workspace; a block of the summaries that a pass cuts goes on from its
    // stored state in the next, with the same additions in the same order
    float* const rows = reinterpret_cast<float*>(ws + l.rows);
    a.f[0].src = rows;
    for (uint64_t r0 = 0; r0 < nframes && e == hipSuccess; r0 += mgx::kTempoChunkRows) {
      const uint64_t cnt = std::min(mgx::kTempoChunkRows, nframes - r0);
      e = mgx::launch_tempogram(env, nframes, f64, table, S, window, W, L, tp.norm, rows, r0, cnt, stream);
      a.row0 = r0;
      a.rows = cnt;
      if (e == hipSuccess) e = mgx::launch_summary_partial(a, stream);
    }
  }
  if (e == hipSuccess) e = mgx::launch_summary_final(a, stream);
  if (e == hipSuccess && lag) e = mgx::launch_tempo_pick(a.f[0].dst, prior, tp.gain, L, S, lag, stream);
  return e;
}

// mgx_summarize_flux_*: the caller's requests, the fields whose rows the call has to hold, and the requests that
// are pooled as the columns of one summary launch (each of width 1; destinations the caller's arrays).
struct FluxReq {
  uint32_t n = 0;
  mgx_flux_request r[MGX_FLUX_MAX_REQUESTS];
  uint32_t cols[MGX_FLUX_MAX_REQUESTS] = {};
  uint32_t rows = 0;
  SummaryFields sf;
  int pooled[MGX_FLUX_MAX_REQUESTS] = {};  // column k of sf is request pooled[k]
  bool any() const { return n != 0; }
};

// (bare: a request may name neither array -- mgx_onsets_host, which reads the column on the device)
int flux_request(const mgx_plan* p, const mgx_flux_request* fr, uint32_t num, uint64_t nsignals, FluxReq* q, bool bare = false) {
  if (num == 0) return MGX_OK;
  if (!fr) return fail(MGX_E_INVALID_ARGUMENT, "flux is NULL with num_flux = %u", num);
  if (num > MGX_FLUX_MAX_REQUESTS) return fail(MGX_E_INVALID_ARGUMENT, "num_flux is %u, at most %d", num, MGX_FLUX_MAX_REQUESTS);
  for (uint32_t i = 0; i < num; ++i) {
    const mgx_flux_request& r = fr[i];
    if (r.struct_size != sizeof(mgx_flux_request))
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_flux_request.struct_size is %u, expected %zu (flux[%u])", r.struct_size,
                  sizeof(mgx_flux_request), i);
    if (r.mode >= MGX_NUM_FLUX_MODES)
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_flux_request.mode is %u, expected 0..%d (flux[%u])", r.mode, MGX_NUM_FLUX_MODES - 1, i);
    if (r.lag < 1 || r.lag > MGX_FLUX_MAX_LAG)
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_flux_request.lag is %u, expected 1..%d (flux[%u])", r.lag, MGX_FLUX_MAX_LAG, i);
    if (!r.per_frame && !r.summary && !bare)
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_flux_request.per_frame and .summary are both NULL (flux[%u])", i);
    if (r.summary && nsignals == 0)
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_flux_request.summary is set with num_signals = 0 (flux[%u])", i);
    if (r.field != MGX_LOUDNESS && r.field != MGX_MFCC && r.field != MGX_AMPLITUDE_SPECTRUM && r.field != MGX_POWER_SPECTRUM &&
        r.field != MGX_MEL_BANDS)
      return fail(MGX_E_UNSUPPORTED, "mgx_flux_request.field is %u: flux is taken of the loudness, mfcc, spectrum and mel_bands rows (flux[%u])",
                  r.field, i);
  }
  q->n = num;
  for (uint32_t i = 0; i < num; ++i) {
    q->r[i] = fr[i];
    q->rows |= 1u << fr[i].field;
    if (p) q->cols[i] = (uint32_t)(mgx::out_field_bytes(p->d, (int)fr[i].field) / 4);
    if (!fr[i].summary) continue;
    mgx::SummaryField& f = q->sf.a.f[q->sf.a.nfields];
    f.dst = fr[i].summary;
    f.width = 1;
    f.col0 = q->sf.a.nfields;
    f.f64 = 0;
    q->pooled[q->sf.a.nfields++] = (int)i;
  }
  q->sf.a.cols = q->sf.a.nfields;
  return MGX_OK;
}

// What the flux requests add to the buffer a summary call works in, from `base` bytes on. Host call: a table and
// per request two carries of lag rows. Both: the flux column of a request the buffer has to hold (device call:
// one without per_frame; host call: every one), the pooling's shifts and partials and (host call) the summaries.
struct FluxLayout {
  uint64_t table, carry[MGX_FLUX_MAX_REQUESTS][2], col[MGX_FLUX_MAX_REQUESTS], shift, part, result, total;
};

FluxLayout flux_layout(const FluxReq& q, uint64_t nframes, uint64_t nsignals, bool host, uint64_t base) {
  FluxLayout l{};
  l.total = base;
  auto take = [&l](uint64_t bytes) {
    const uint64_t at = l.total;
    l.total += (bytes + 255) / 256 * 256;
    return at;
  };
  if (!q.any() || nsignals == 0 || nframes == 0) return l;
  if (host) l.table = take((nsignals + 1) * sizeof(uint64_t));
  for (uint32_t i = 0; i < q.n; ++i) {
    if (host)
      for (int k = 0; k < 2; ++k) l.carry[i][k] = take((uint64_t)q.r[i].lag * q.cols[i] * sizeof(float));
    l.col[i] = host || !q.r[i].per_frame ? take(nframes * sizeof(float)) : UINT64_MAX;
  }
  const uint64_t cols = q.sf.a.cols;
  l.shift = take(nsignals * cols * sizeof(double));
  l.part = take((nframes / mgx::kSummaryBlock + nsignals + 1) * mgx::kSummaryWords * cols * sizeof(double));
  if (host) l.result = take(nsignals * MGX_NUM_STATS * cols * sizeof(double));
  return l;
}

// The pooling of the flux columns col[i] (nframes floats each, device memory) into the destinations of q.sf
int flux_pool(FluxReq& q, float* const* col, unsigned char* buf, const FluxLayout& l, const uint64_t* table, uint64_t nframes,
              uint64_t nsignals, hipStream_t st) {
  mgx::SummaryArgs& a = q.sf.a;
  if (a.cols == 0) return MGX_OK;
  for (uint32_t k = 0; k < a.nfields; ++k) a.f[k].src = col[q.pooled[k]];
  a.num_signals = nsignals;
  a.num_frames = nframes;
  a.table = table;
  a.shift = reinterpret_cast<double*>(buf + l.shift);
  a.part = reinterpret_cast<double*>(buf + l.part);
  a.row0 = 0;
  a.rows = nframes;
  a.slot0 = 0;
  a.nslots = nframes / mgx::kSummaryBlock + nsignals;
  hipError_t e = mgx::launch_summary_partial(a, st);
  if (e == hipSuccess) e = mgx::launch_summary_final(a, st);
  return e == hipSuccess ? (int)MGX_OK : hip_fail(e, "summary kernel launch");
}

int summarize_host_impl(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                        const uint64_t* frame_offsets, uint64_t nsignals, const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                        const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas,
                        const mgx_flux_request* flux = nullptr, uint32_t nflux = 0, const PeakHost* pick = nullptr,
                        const TempoHost* tempo = nullptr);

// mgx_summarize_deltas_workspace_bytes (deltas there, no request) and mgx_summarize_flux_workspace_bytes (deltas or
// not, requests): the summary call's buffer with the rows of every delta'd or flux'd field kept, then what the
// deltas and the flux add.
int summarize_more_workspace_bytes(const mgx_plan* p, const mgx_outputs* o, const mgx_aux_outputs* aux, const mgx_summary_outputs* summary,
                                   const mgx_delta_summaries* deltas, const mgx_flux_request* flux, uint32_t nflux, uint64_t nframes,
                                   uint64_t nsignals, uint64_t* bytes) {
  if (!bytes) return fail(MGX_E_INVALID_ARGUMENT, "bytes is NULL");
  const mgx_outputs none{};
  mgx::Outputs x;
  DeltaReq q;
  FluxReq fq;
  int rc = check_summary(summary);
  if (rc || (rc = delta_request(p, deltas, &q)) || (rc = flux_request(p, flux, nflux, nsignals, &fq)) ||
      (rc = make_outputs(p, o ? o : &none, aux, &x)))
    return rc;
  SummaryFields sf;
  summary_fields(p, summary, &sf);
  const uint32_t extra = (sf.pooled | q.rows[0] | fq.rows) & ~mgx::out_requested(x);
  const SummaryLayout l = summary_layout(p->d, extra, sf.a.cols, nframes, nsignals, false, q.any() || fq.any());
  const DeltaLayout dl = delta_layout(p->d, q, nframes, nsignals, false, l.total);
  *bytes = flux_layout(fq, nframes, nsignals, false, dl.total).total;
  return MGX_OK;
}

// The device call of the same two: the gather launch and the base pooling as mgx_summarize_device makes them, then
// the deltas (delta_pool), then the flux operator per request and the pooling of its columns.
int summarize_more_device(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                          const uint64_t* frame_offsets, uint64_t nsignals, const mgx_outputs* o, const mgx_aux_outputs* aux,
                          const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas, const mgx_flux_request* flux,
                          uint32_t nflux, void* workspace, uint64_t workspace_bytes, void* stream) {
  const mgx_outputs none{};
  mgx::Outputs x;
  DeltaReq q;
  FluxReq fq;
  int rc = check_summary(summary);
  if (rc || (rc = delta_request(p, deltas, &q)) || (rc = flux_request(p, flux, nflux, nsignals, &fq)) ||
      (rc = make_outputs(p, o ? o : &none, aux, &x)))
    return rc;
  if (!q.any() && !fq.any())  // (no field named in either struct, no request: the summary call)
    return mgx_summarize_device(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, o, aux, summary, workspace,
                                workspace_bytes, stream);
  SummaryFields sf;
  summary_fields(p, summary, &sf);
  if ((rc = summary_inputs(p, samples, num_samples, starts, nframes, frame_offsets, nsignals))) return rc;
  if ((rc = check_outputs(x))) return rc;
  const uint32_t extra = (sf.pooled | q.rows[0] | fq.rows) & ~mgx::out_requested(x);
  const SummaryLayout l = summary_layout(p->d, extra, sf.a.cols, nframes, nsignals, false, true);
  const DeltaLayout dl = delta_layout(p->d, q, nframes, nsignals, false, l.total);
  const FluxLayout fl = flux_layout(fq, nframes, nsignals, false, dl.total);
  if (workspace_bytes < fl.total || (fl.total > 0 && !workspace))
    return fail(MGX_E_INVALID_ARGUMENT, "the workspace holds %llu bytes, the call needs %llu (%s)", (unsigned long long)workspace_bytes,
                (unsigned long long)fl.total, fq.any() ? "mgx_summarize_flux_workspace_bytes" : "mgx_summarize_deltas_workspace_bytes");
  if (fl.total > 0 && reinterpret_cast<uintptr_t>(workspace) % 256 != 0)
    return fail(MGX_E_INVALID_ARGUMENT, "the workspace is not 256-byte aligned");
  unsigned char* const ws = static_cast<unsigned char*>(workspace);
  // the launch's outputs: the caller's per-frame arrays, and for the other pooled, delta'd or flux'd fields the workspace's
  mgx::Outputs u = x;
  if (l.total > 0)
    for (int i = 0; i < mgx::kOutFields; ++i)
      if (l.frames[i] != UINT64_MAX) mgx::out_field(u, i) = ws + l.frames[i];
  if (nframes > 0) {
    const GatherLaunch g{starts, num_samples};
    LaunchOpts opt;
    opt.gather = &g;
    if ((rc = extract_device_impl(p, samples, nframes, (uint64_t)p->n, l.total > 0 ? &u : &x, stream, opt))) return rc;
  }
  if (nsignals == 0) return MGX_OK;  // (no signal owns a row: the gather call, no flux written)
  hipError_t e = hipSetDevice(p->d.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  mgx::SummaryArgs& a = sf.a;
  a.num_signals = nsignals;
  a.num_frames = nframes;
  uint64_t* const table = nframes > 0 ? reinterpret_cast<uint64_t*>(ws + l.table) : nullptr;
  if (nframes > 0) {
    // the base summaries, exactly as mgx_summarize_device forms them; the table serves the deltas and the flux too
    for (uint32_t i = 0; i < a.nfields; ++i) a.f[i].src = mgx::out_field(u, sf.index[i]);
    a.table = table;
    a.shift = reinterpret_cast<double*>(ws + l.shift);
    a.part = reinterpret_cast<double*>(ws + l.part);
    a.row0 = 0;
    a.rows = nframes;
    a.slot0 = 0;
    a.nslots = nframes / mgx::kSummaryBlock + nsignals;
    e = mgx::launch_summary_table(frame_offsets, table, nsignals, nframes, (hipStream_t)stream);
    if (e == hipSuccess) e = mgx::launch_summary_partial(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "summary kernel launch");
  }
  e = mgx::launch_summary_final(a, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "summary kernel launch");
  if (nframes == 0) {
    // no buffers: every signal is empty, NaN in all four (the final kernel reads neither rows nor table)
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
      q.sf[k].a.num_signals = nsignals;
      q.sf[k].a.num_frames = 0;
      e = mgx::launch_summary_final(q.sf[k].a, (hipStream_t)stream);
    }
    fq.sf.a.num_signals = nsignals;
    fq.sf.a.num_frames = 0;
    if (e == hipSuccess) e = mgx::launch_summary_final(fq.sf.a, (hipStream_t)stream);
    return e == hipSuccess ? (int)MGX_OK : hip_fail(e, "summary kernel launch");
  }
  if (q.any() && (rc = delta_pool(p->d, q, u, ws, dl, table, nframes, nsignals, (hipStream_t)stream))) return rc;
  if (!fq.any()) return MGX_OK;
  // the operator per request over the field's rows, then the pooling of the one-column flux arrays
  float* col[MGX_FLUX_MAX_REQUESTS];
  for (uint32_t i = 0; i < fq.n; ++i) {
    col[i] = fq.r[i].per_frame ? fq.r[i].per_frame : reinterpret_cast<float*>(ws + fl.col[i]);
    e = mgx::launch_flux(mgx::out_field(u, (int)fq.r[i].field), nullptr, col[i], 0, nframes, nframes, fq.cols[i], false, table, nsignals,
                         fq.r[i].mode, fq.r[i].lag, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "flux kernel launch");
  }
  return flux_pool(fq, col, ws, fl, table, nframes, nsignals, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int mgx_delta_device(const void* rows, uint64_t num_frames, uint32_t cols, uint32_t rows_f64, const uint64_t* frame_offsets,
                     uint64_t num_signals, uint32_t width, void* delta, void* delta2, void* stream) {
  if (cols == 0) return fail(MGX_E_INVALID_ARGUMENT, "cols is 0");
  if (width < 1 || width > MGX_DELTA_MAX_WIDTH)
    return fail(MGX_E_INVALID_ARGUMENT, "width is %u, expected 1..%d", width, MGX_DELTA_MAX_WIDTH);
  if (rows_f64 > 1) return fail(MGX_E_INVALID_ARGUMENT, "rows_f64 is %u, expected 0 or 1", rows_f64);
  if (!delta && !delta2) return fail(MGX_E_INVALID_ARGUMENT, "delta and delta2 are both NULL");
  if (delta == delta2) return fail(MGX_E_INVALID_ARGUMENT, "delta and delta2 are the same array");
  if (rows && (delta == rows || delta2 == rows)) return fail(MGX_E_INVALID_ARGUMENT, "an output is the rows' own array");
  if (num_signals > 0 && !frame_offsets) return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets is NULL");
  if (num_frames == 0) return MGX_OK;
  if (!rows) return fail(MGX_E_INVALID_ARGUMENT, "rows is NULL");
  // (frame_offsets with num_signals = 0: a table of one entry, no signal, nothing written)
  hipError_t e = hipSuccess;
  if (delta) {
    e = mgx::launch_delta(rows, delta, num_frames, cols, rows_f64 != 0, frame_offsets, num_signals, width, false, (hipStream_t)stream);
    if (e == hipSuccess && delta2)
      e = mgx::launch_delta(delta, delta2, num_frames, cols, rows_f64 != 0, frame_offsets, num_signals, width, false, (hipStream_t)stream);
  } else {
    // no array for the delta rows: each one is recomputed where the second order reads it
    e = mgx::launch_delta(rows, delta2, num_frames, cols, rows_f64 != 0, frame_offsets, num_signals, width, true, (hipStream_t)stream);
  }
  return e == hipSuccess ? MGX_OK : hip_fail(e, "delta kernel launch");
}

int mgx_summarize_deltas_workspace_bytes(const mgx_plan* p, const mgx_outputs* o, const mgx_aux_outputs* aux,
                                         const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas, uint64_t nframes,
                                         uint64_t nsignals, uint64_t* bytes) {
  if (!deltas) return mgx_summary_workspace_bytes(p, o, aux, summary, nframes, nsignals, bytes);
  return summarize_more_workspace_bytes(p, o, aux, summary, deltas, nullptr, 0, nframes, nsignals, bytes);
}

int mgx_summarize_deltas_device(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                                const uint64_t* frame_offsets, uint64_t nsignals, const mgx_outputs* o, const mgx_aux_outputs* aux,
                                const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas, void* workspace,
                                uint64_t workspace_bytes, void* stream) {
  if (!deltas)
    return mgx_summarize_device(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, o, aux, summary, workspace,
                                workspace_bytes, stream);
  return summarize_more_device(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, o, aux, summary, deltas, nullptr, 0,
                               workspace, workspace_bytes, stream);
}

int mgx_summarize_deltas_host(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                              const uint64_t* frame_offsets, uint64_t nsignals, const mgx_outputs* outputs,
                              const mgx_aux_outputs* aux, const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas) {
  return summarize_host_impl(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, outputs, aux, summary, deltas);
}

int mgx_flux_device(const void* rows, uint64_t num_frames, uint32_t cols, uint32_t rows_f64, const uint64_t* frame_offsets,
                    uint64_t num_signals, uint32_t mode, uint32_t lag, void* flux, void* stream) {
  if (cols == 0) return fail(MGX_E_INVALID_ARGUMENT, "cols is 0");
  if (mode >= MGX_NUM_FLUX_MODES) return fail(MGX_E_INVALID_ARGUMENT, "mode is %u, expected 0..%d", mode, MGX_NUM_FLUX_MODES - 1);
  if (lag < 1 || lag > MGX_FLUX_MAX_LAG) return fail(MGX_E_INVALID_ARGUMENT, "lag is %u, expected 1..%d", lag, MGX_FLUX_MAX_LAG);
  if (rows_f64 > 1) return fail(MGX_E_INVALID_ARGUMENT, "rows_f64 is %u, expected 0 or 1", rows_f64);
  if (!flux) return fail(MGX_E_INVALID_ARGUMENT, "flux is NULL");
  if (flux == rows) return fail(MGX_E_INVALID_ARGUMENT, "flux is the rows' own array");
  if (num_signals > 0 && !frame_offsets) return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets is NULL");
  if (num_frames == 0) return MGX_OK;
  if (!rows) return fail(MGX_E_INVALID_ARGUMENT, "rows is NULL");
  // (frame_offsets with num_signals = 0: a table of one entry, no signal, nothing written)
  const hipError_t e = mgx::launch_flux(rows, nullptr, flux, 0, num_frames, num_frames, cols, rows_f64 != 0, frame_offsets, num_signals,
                                        mode, lag, (hipStream_t)stream);
  return e == hipSuccess ? MGX_OK : hip_fail(e, "flux kernel launch");
}

int mgx_summarize_flux_workspace_bytes(const mgx_plan* p, const mgx_outputs* o, const mgx_aux_outputs* aux,
                                       const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas,
                                       const mgx_flux_request* flux, uint32_t nflux, uint64_t nframes, uint64_t nsignals,
                                       uint64_t* bytes) {
  if (nflux == 0) return mgx_summarize_deltas_workspace_bytes(p, o, aux, summary, deltas, nframes, nsignals, bytes);
  return summarize_more_workspace_bytes(p, o, aux, summary, deltas, flux, nflux, nframes, nsignals, bytes);
}

int mgx_summarize_flux_device(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                              const uint64_t* frame_offsets, uint64_t nsignals, const mgx_outputs* o, const mgx_aux_outputs* aux,
                              const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas, const mgx_flux_request* flux,
                              uint32_t nflux, void* workspace, uint64_t workspace_bytes, void* stream) {
  if (nflux == 0)
    return mgx_summarize_deltas_device(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, o, aux, summary, deltas,
                                       workspace, workspace_bytes, stream);
  return summarize_more_device(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, o, aux, summary, deltas, flux, nflux,
                               workspace, workspace_bytes, stream);
}

int mgx_peaks_workspace_bytes(uint64_t num_frames, uint64_t num_signals, uint64_t* bytes) {
  (void)num_signals;  // (the bitmaps are the rows': a table costs nothing)
  if (!bytes) return fail(MGX_E_INVALID_ARGUMENT, "bytes is NULL");
  *bytes = mgx::peaks_workspace_bytes(num_frames);
  return MGX_OK;
}

int mgx_peaks_device(const void* envelope, uint64_t num_frames, uint32_t envelope_f64, const uint64_t* frame_offsets,
                     uint64_t num_signals, const mgx_peak_params* params, const mgx_peak_outputs* out, void* workspace,
                     uint64_t workspace_bytes, void* stream) {
  int rc = check_peak_params(params);
  if (rc) return rc;
  if (!out) return fail(MGX_E_INVALID_ARGUMENT, "out is NULL");
  if (out->struct_size != sizeof(mgx_peak_outputs))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.struct_size is %u, expected %zu", out->struct_size, sizeof(mgx_peak_outputs));
  if (envelope_f64 > 1) return fail(MGX_E_INVALID_ARGUMENT, "envelope_f64 is %u, expected 0 or 1", envelope_f64);
  if (!out->mask && !out->peak_offsets && !out->peaks)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.mask, .peak_offsets and .peaks are all NULL");
  if (out->peaks && out->capacity == 0) return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.peaks is set with capacity 0");
  if (out->peak_starts && !out->starts) return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.peak_starts is set without starts");
  if (out->peak_starts && !out->peaks) return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.peak_starts is set without peaks");
  if (num_signals > 0 && !frame_offsets) return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets is NULL");
  if (num_frames > 0 && !envelope) return fail(MGX_E_INVALID_ARGUMENT, "envelope is NULL");
  const uint64_t need = mgx::peaks_workspace_bytes(num_frames);
  if (workspace_bytes < need || (need > 0 && !workspace))
    return fail(MGX_E_INVALID_ARGUMENT, "the workspace holds %llu bytes, the call needs %llu (mgx_peaks_workspace_bytes)",
                (unsigned long long)workspace_bytes, (unsigned long long)need);
  if (need > 0 && reinterpret_cast<uintptr_t>(workspace) % 256 != 0)
    return fail(MGX_E_INVALID_ARGUMENT, "the workspace is not 256-byte aligned");
  if (num_frames == 0) {
    // no rows, no peaks: the offsets alone (frame_offsets with num_signals = 0: no signal, one entry)
    if (!out->peak_offsets) return MGX_OK;
    const uint64_t S = frame_offsets ? num_signals : 1;
    const hipError_t e = hipMemsetAsync(out->peak_offsets, 0, (S + 1) * sizeof(uint64_t), (hipStream_t)stream);
    return e == hipSuccess ? MGX_OK : hip_fail(e, "hipMemsetAsync(peak_offsets)");
  }
  const hipError_t e = mgx::launch_peaks(envelope, num_frames, envelope_f64 != 0, frame_offsets, num_signals, *params, *out, workspace,
                                         (hipStream_t)stream);
  return e == hipSuccess ? MGX_OK : hip_fail(e, "peak kernel launch");
}

int mgx_onsets_host(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                    const uint64_t* frame_offsets, uint64_t nsignals, const mgx_flux_request* flux, const mgx_peak_params* params,
                    uint64_t* peak_offsets, uint64_t* peaks, uint64_t capacity) {
  int rc = check_peak_params(params);
  if (rc) return rc;
  if (nsignals == 0) return fail(MGX_E_INVALID_ARGUMENT, "num_signals is 0: onsets are picked within signals");
  if (!flux) return fail(MGX_E_INVALID_ARGUMENT, "flux is NULL");
  if (!peak_offsets) return fail(MGX_E_INVALID_ARGUMENT, "peak_offsets is NULL");
  if (!peaks && capacity > 0) return fail(MGX_E_INVALID_ARGUMENT, "peaks is NULL with capacity %llu", (unsigned long long)capacity);
  if (peaks && capacity == 0) return fail(MGX_E_INVALID_ARGUMENT, "peaks is set with capacity 0");
  mgx_summary_outputs none{};
  none.struct_size = sizeof(none);
  const PeakHost pick{params, peak_offsets, peaks, capacity};
  return summarize_host_impl(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, nullptr, nullptr, &none, nullptr, flux, 1,
                             &pick);
}

int mgx_summarize_flux_host(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                            const uint64_t* frame_offsets, uint64_t nsignals, const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                            const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas, const mgx_flux_request* flux,
                            uint32_t nflux) {
  return summarize_host_impl(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, outputs, aux, summary, deltas, flux,
                             nflux);
}

int mgx_summary_workspace_bytes(const mgx_plan* p, const mgx_outputs* o, const mgx_aux_outputs* aux, const mgx_summary_outputs* summary,
                                uint64_t nframes, uint64_t nsignals, uint64_t* bytes) {
  if (!bytes) return fail(MGX_E_INVALID_ARGUMENT, "bytes is NULL");
  const mgx_outputs none{};
  mgx::Outputs x;
  int rc = check_summary(summary);
  if (rc || (rc = make_outputs(p, o ? o : &none, aux, &x))) return rc;
  SummaryFields sf;
  summary_fields(p, summary, &sf);
  *bytes = summary_layout(p->d, sf.pooled & ~mgx::out_requested(x), sf.a.cols, nframes, nsignals, false).total;
  return MGX_OK;
}

int mgx_summarize_device(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                         const uint64_t* frame_offsets, uint64_t nsignals, const mgx_outputs* o, const mgx_aux_outputs* aux,
                         const mgx_summary_outputs* summary, void* workspace, uint64_t workspace_bytes, void* stream) {
  const mgx_outputs none{};
  mgx::Outputs x;
  int rc = check_summary(summary);
  if (rc || (rc = make_outputs(p, o ? o : &none, aux, &x))) return rc;
  SummaryFields sf;
  summary_fields(p, summary, &sf);
  if ((rc = summary_inputs(p, samples, num_samples, starts, nframes, frame_offsets, nsignals))) return rc;
  if ((rc = check_outputs(x))) return rc;
  const SummaryLayout l = summary_layout(p->d, sf.pooled & ~mgx::out_requested(x), sf.a.cols, nframes, nsignals, false);
  if (workspace_bytes < l.total || (l.total > 0 && !workspace))
    return fail(MGX_E_INVALID_ARGUMENT, "the workspace holds %llu bytes, the call needs %llu (mgx_summary_workspace_bytes)",
                (unsigned long long)workspace_bytes, (unsigned long long)l.total);
  if (l.total > 0 && reinterpret_cast<uintptr_t>(workspace) % 256 != 0)
    return fail(MGX_E_INVALID_ARGUMENT, "the workspace is not 256-byte aligned");
  unsigned char* const ws = static_cast<unsigned char*>(workspace);
  // the launch's outputs: the caller's per-frame arrays, and for the other pooled fields the workspace's
  mgx::Outputs u = x;
  if (l.total > 0)
    for (int i = 0; i < mgx::kOutFields; ++i)
      if (l.frames[i] != UINT64_MAX) mgx::out_field(u, i) = ws + l.frames[i];
  if (nframes > 0) {
    const GatherLaunch g{starts, num_samples};
    LaunchOpts opt;
    opt.gather = &g;
    // (with nothing to pool for, the launch writes the caller's fields alone: the gather call)
    if ((rc = extract_device_impl(p, samples, nframes, (uint64_t)p->n, l.total > 0 ? &u : &x, stream, opt))) return rc;
  }
  if (nsignals == 0 || sf.a.cols == 0) return MGX_OK;
  hipError_t e = hipSetDevice(p->d.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  mgx::SummaryArgs& a = sf.a;
  a.num_signals = nsignals;
  a.num_frames = nframes;
  if (nframes > 0) {
    for (uint32_t i = 0; i < a.nfields; ++i) a.f[i].src = mgx::out_field(u, sf.index[i]);
    uint64_t* const table = reinterpret_cast<uint64_t*>(ws + l.table);
    a.table = table;
    a.shift = reinterpret_cast<double*>(ws + l.shift);
    a.part = reinterpret_cast<double*>(ws + l.part);
    a.row0 = 0;
    a.rows = nframes;
    a.slot0 = 0;
    a.nslots = nframes / mgx::kSummaryBlock + nsignals;
    e = mgx::launch_summary_table(frame_offsets, table, nsignals, nframes, (hipStream_t)stream);
    if (e == hipSuccess) e = mgx::launch_summary_partial(a, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "summary kernel launch");
  }
  e = mgx::launch_summary_final(a, (hipStream_t)stream);
  return e == hipSuccess ? MGX_OK : hip_fail(e, "summary kernel launch");
}

int mgx_summarize_host(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                       const uint64_t* frame_offsets, uint64_t nsignals, const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                       const mgx_summary_outputs* summary) {
  return summarize_host_impl(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, outputs, aux, summary, nullptr);
}

}  // extern "C"

namespace {

// mgx_summarize_host (deltas null: nothing here differs from what it was), mgx_summarize_deltas_host and
// mgx_summarize_flux_host (no request: nothing here differs from the deltas call)
int summarize_host_impl(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                        const uint64_t* frame_offsets, uint64_t nsignals, const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                        const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas, const mgx_flux_request* flux,
                        uint32_t nflux, const PeakHost* pick, const TempoHost* tempo) {
  const mgx_outputs none{};
  mgx::Outputs x;
  DeltaReq q;
  FluxReq fq;
  int rc = check_summary(summary);
  if (rc || (rc = delta_request(p, deltas, &q)) || (rc = flux_request(p, flux, nflux, nsignals, &fq, pick != nullptr || tempo != nullptr)) ||
      (rc = make_outputs(p, outputs ? outputs : &none, aux, &x)))
    return rc;
  SummaryFields sf;
  summary_fields(p, summary, &sf);
  if ((rc = summary_inputs(p, samples, num_samples, starts, nframes, frame_offsets, nsignals))) return rc;
  if ((rc = check_outputs(x))) return rc;
  // (the host sees both tables: they are checked here, before any copy)
  const uint64_t n = (uint64_t)p->n;
  for (uint64_t f = 0; f < nframes; ++f)
    if (starts[f] > num_samples - n)
      return fail(MGX_E_INVALID_ARGUMENT, "starts[%llu] = %llu: a buffer of %d leaves the %llu samples", (unsigned long long)f,
                  (unsigned long long)starts[f], p->n, (unsigned long long)num_samples);
  for (uint64_t s = 0; s < nsignals; ++s)
    if (frame_offsets[s + 1] < frame_offsets[s])
      return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets[%llu] = %llu is below frame_offsets[%llu] = %llu", (unsigned long long)(s + 1),
                  (unsigned long long)frame_offsets[s + 1], (unsigned long long)s, (unsigned long long)frame_offsets[s]);
  if (nsignals > 0 && frame_offsets[nsignals] > nframes)
    return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets[%llu] = %llu is above the %llu buffers", (unsigned long long)nsignals,
                (unsigned long long)frame_offsets[nsignals], (unsigned long long)nframes);
  resident_stop(p);
  mgx::SummaryArgs& a = sf.a;
  if (nframes == 0) {
    // no buffers: every signal is empty, NaN in all four (nothing for the device to do)
    for (uint32_t i = 0; i < a.nfields; ++i)
      std::fill_n(a.f[i].dst, nsignals * MGX_NUM_STATS * a.f[i].width, std::nan(""));
    for (int k = 0; k < 2; ++k)
      for (uint32_t i = 0; i < q.sf[k].a.nfields; ++i)
        std::fill_n(q.sf[k].a.f[i].dst, nsignals * MGX_NUM_STATS * q.sf[k].a.f[i].width, std::nan(""));
    for (uint32_t i = 0; i < fq.sf.a.nfields; ++i) std::fill_n(fq.sf.a.f[i].dst, nsignals * MGX_NUM_STATS, std::nan(""));
    if (pick) std::fill_n(pick->peak_offsets, nsignals + 1, (uint64_t)0);
    if (tempo && tempo->summary) std::fill_n(tempo->summary, nsignals * MGX_NUM_STATS * tempo->params->num_lags, std::nan(""));
    if (tempo && tempo->lag) std::fill_n(tempo->lag, nsignals, (uint32_t)0);
    if (tempo && tempo->beats) std::fill_n(tempo->beats->peak_offsets, nsignals + 1, (uint64_t)0);
    return MGX_OK;
  }
  if (nsignals == 0 || (a.cols == 0 && !q.any() && !fq.any())) return gather_host_chunked(p, samples, starts, nframes, &x, nullptr);
  const SummaryLayout l = summary_layout(p->d, 0, a.cols, nframes, nsignals, true);
  hipError_t e = hipSetDevice(p->d.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  // the staging streams first: the table's copy and the last kernel go on the compute stream
  if ((rc = ensure_host_staging(p, 1, mgx::kOutLayoutSlack))) return rc;
  if (p->s_sum_bytes < l.total) {
    if (p->s_sum) (void)hipFree(p->s_sum);
    p->s_sum = nullptr;
    p->s_sum_bytes = 0;
    e = hipMalloc(reinterpret_cast<void**>(&p->s_sum), l.total);
    if (e != hipSuccess) { p->s_sum = nullptr; return hip_fail(e, "hipMalloc(summary buffers)"); }
    p->s_sum_bytes = l.total;
  }
  // the deltas' own buffer: the delta'd fields' rows of the whole call (each chunk's copied in behind its
  // extraction), then what delta_layout adds
  uint64_t xoff[mgx::kOutFields];
  const DeltaLayout dl = delta_layout(p->d, q, nframes, nsignals, true, mgx::out_layout(p->d, q.rows[0], nframes, xoff));
  if (q.any() && p->s_delta_bytes < dl.total) {
    if (p->s_delta) (void)hipFree(p->s_delta);
    p->s_delta = nullptr;
    p->s_delta_bytes = 0;
    e = hipMalloc(reinterpret_cast<void**>(&p->s_delta), dl.total);
    if (e != hipSuccess) { p->s_delta = nullptr; return hip_fail(e, "hipMalloc(delta rows)"); }
    p->s_delta_bytes = dl.total;
  }
  // the flux's own buffer: no rows but the carries, and the flux columns of the whole call
  const FluxLayout fl = flux_layout(fq, nframes, nsignals, true, 0);
  // behind it, for mgx_onsets_host: the picker's workspace, its offsets and the peaks the caller has room for
  const uint64_t pick_ws = fl.total, pick_ws_bytes = pick ? mgx::peaks_workspace_bytes(nframes) : 0;
  const uint64_t pick_off = pick_ws + pick_ws_bytes, pick_off_bytes = pick ? ((nsignals + 1) * 8 + 255) / 256 * 256 : 0;
  const uint64_t pick_cap = pick && pick->peaks ? std::min(pick->capacity, nframes) : 0;
  const uint64_t pick_peaks = pick_off + pick_off_bytes, flux_total = pick_peaks + (pick_cap * 8 + 255) / 256 * 256;
  if (fq.any() && p->s_flux_bytes < flux_total) {
    if (p->s_flux) (void)hipFree(p->s_flux);
    p->s_flux = nullptr;
    p->s_flux_bytes = 0;
    e = hipMalloc(reinterpret_cast<void**>(&p->s_flux), flux_total);
    if (e != hipSuccess) { p->s_flux = nullptr; return hip_fail(e, "hipMalloc(flux columns)"); }
    p->s_flux_bytes = flux_total;
  }
  // mgx_tempo_host's own buffer: the window, the prior, the workspace of mgx_tempo_device and the lags
  const uint32_t tempo_L = tempo ? tempo->params->num_lags : 0;
  const uint64_t tempo_win = 0, tempo_prior = MGX_TEMPOGRAM_MAX_WIN * sizeof(float);
  const uint64_t tempo_ws = tempo_prior + MGX_TEMPOGRAM_MAX_WIN * sizeof(double);
  const uint64_t tempo_lag = tempo_ws + (tempo ? tempo_layout(nframes, nsignals, tempo_L, false).total : 0);
  // behind them, for mgx_beats_host: the two tables, the tracker's workspace, its offsets and the beats there is room for
  const BeatHost* const beats = tempo ? tempo->beats : nullptr;
  auto up256 = [](uint64_t bytes) { return (bytes + 255) / 256 * 256; };
  const uint32_t beat_P = beats ? beats->params->max_period : 0;
  const uint64_t beat_gauss = tempo_lag + up256(nsignals * sizeof(uint32_t));
  const uint64_t beat_pen = beat_gauss + (beats ? up256(beat_gauss_count(beat_P) * sizeof(float)) : 0);
  const uint64_t beat_ws = beat_pen + (beats ? up256(beat_penalty_count(beat_P) * sizeof(double)) : 0);
  const uint64_t beat_off = beat_ws + (beats ? mgx::beats_workspace_bytes(nframes, nsignals) : 0);
  const uint64_t beat_cap = beats && beats->peaks ? std::min(beats->capacity, nframes) : 0;
  const uint64_t beat_rows = beat_off + (beats ? up256((nsignals + 1) * 8) : 0);
  const uint64_t tempo_total = beat_rows + up256(beat_cap * 8);
  if (tempo && p->s_tempo_bytes < tempo_total) {
    if (p->s_tempo) (void)hipFree(p->s_tempo);
    p->s_tempo = nullptr;
    p->s_tempo_bytes = 0;
    e = hipMalloc(reinterpret_cast<void**>(&p->s_tempo), tempo_total);
    if (e != hipSuccess) { p->s_tempo = nullptr; return hip_fail(e, "hipMalloc(tempo buffers)"); }
    p->s_tempo_bytes = tempo_total;
  }
  if (fq.any()) {
    e = hipMemcpyAsync(p->s_flux + fl.table, frame_offsets, (nsignals + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p->s_comp);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(frame_offsets)");
  }
  int carry_now = 0;  // which of a request's two carries holds the rows before the next chunk
  a.num_signals = nsignals;
  a.num_frames = nframes;
  if (a.cols > 0) {
    a.table = reinterpret_cast<const uint64_t*>(p->s_sum + l.table);
    a.shift = reinterpret_cast<double*>(p->s_sum + l.shift);
    a.part = reinterpret_cast<double*>(p->s_sum + l.part);
    e = hipMemcpyAsync(p->s_sum + l.table, frame_offsets, (nsignals + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p->s_comp);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(frame_offsets)");
  }
  if (q.any()) {
    e = hipMemcpyAsync(p->s_delta + dl.table, frame_offsets, (nsignals + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p->s_comp);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(frame_offsets)");
  }
  ChunkHook hook;
  hook.pooled = sf.pooled | q.rows[0] | fq.rows;
  auto reduce_chunk = [&](uint64_t f0, uint64_t cnt, const mgx::Outputs& d) {
    // the chunk's rows [f0, f0 + cnt) and the slots they can belong to: from the block that holds the first of
    // them that a signal owns to the block that holds the last (the kernel passes over a slot without rows here)
    const uint64_t* const tb = frame_offsets;
    const uint64_t c0 = f0, c1 = f0 + cnt, B = mgx::kSummaryBlock;
    const uint64_t* const it = std::upper_bound(tb + 1, tb + nsignals + 1, c0);  // the first signal that ends after c0
    if (it == tb + nsignals + 1) return (int)MGX_OK;
    const uint64_t s_lo = (uint64_t)(it - (tb + 1)), a_lo = tb[s_lo];
    if (a_lo >= c1) return (int)MGX_OK;
    const uint64_t s_hi = (uint64_t)(std::lower_bound(tb, tb + nsignals, c1) - tb) - 1;  // the last signal that begins before c1
    const uint64_t a_hi = tb[s_hi], e_hi = std::min(c1, tb[s_hi + 1]), last = e_hi > a_hi ? e_hi - 1 : a_hi;
    mgx::SummaryArgs c = a;
    for (uint32_t i = 0; i < c.nfields; ++i) c.f[i].src = mgx::out_field(d, sf.index[i]);
    c.row0 = c0;
    c.rows = cnt;
    c.slot0 = a_lo / B + s_lo + (std::max(c0, a_lo) - a_lo) / B;
    c.nslots = a_hi / B + s_hi + (last - a_hi) / B - c.slot0 + 1;
    const hipError_t ke = mgx::launch_summary_partial(c, p->s_comp);
    return ke == hipSuccess ? (int)MGX_OK : hip_fail(ke, "summary kernel launch");
  };
  hook.after = [&](uint64_t f0, uint64_t cnt, const mgx::Outputs& d) {
    if (a.cols > 0) {
      const int hr = reduce_chunk(f0, cnt, d);
      if (hr) return hr;
    }
    // the delta'd fields' rows of the chunk to their place in the call's arrays, before the slot is reused
    hipError_t ce = hipSuccess;
    for (int i = 0; i < mgx::kOutFields && ce == hipSuccess; ++i) {
      if (!((q.rows[0] >> i) & 1u)) continue;
      const uint64_t fb = mgx::out_field_bytes(p->d, i);
      ce = hipMemcpyAsync(p->s_delta + xoff[i] + f0 * fb, mgx::out_field(d, i), cnt * fb, hipMemcpyDeviceToDevice, p->s_comp);
    }
    if (ce != hipSuccess) return hip_fail(ce, "hipMemcpyAsync(delta rows)");
    // the chunk's flux over the slot's rows and the carry, into the call's columns; then the chunk's last lag rows
    // (behind what is left of the carry, when the chunk has fewer) into the other carry, before the slot is reused
    for (uint32_t i = 0; i < fq.n && ce == hipSuccess; ++i) {
      const uint64_t lag = fq.r[i].lag, rb = (uint64_t)fq.cols[i] * sizeof(float);
      const unsigned char* const rows = static_cast<const unsigned char*>(mgx::out_field(d, (int)fq.r[i].field));
      unsigned char* const now = p->s_flux + fl.carry[i][carry_now];
      unsigned char* const next = p->s_flux + fl.carry[i][carry_now ^ 1];
      ce = mgx::launch_flux(rows, f0 > 0 ? now : nullptr, reinterpret_cast<float*>(p->s_flux + fl.col[i]) + f0, f0, cnt, nframes,
                            fq.cols[i], false, reinterpret_cast<const uint64_t*>(p->s_flux + fl.table), nsignals, fq.r[i].mode,
                            fq.r[i].lag, p->s_comp);
      const uint64_t keep = cnt < lag ? lag - cnt : 0, take = lag - keep;
      if (ce == hipSuccess && keep > 0) ce = hipMemcpyAsync(next, now + (lag - keep) * rb, keep * rb, hipMemcpyDeviceToDevice, p->s_comp);
      if (ce == hipSuccess)
        ce = hipMemcpyAsync(next + keep * rb, rows + (cnt - take) * rb, take * rb, hipMemcpyDeviceToDevice, p->s_comp);
    }
    carry_now ^= 1;
    return ce == hipSuccess ? (int)MGX_OK : hip_fail(ce, "flux kernel launch and carry copies");
  };
  if ((rc = gather_host_chunked(p, samples, starts, nframes, &x, &hook))) return rc;
  // the signals' partials into the summaries, and those alone back to the caller
  double* const result = reinterpret_cast<double*>(p->s_sum + l.result);
  std::vector<double*> host_dst(a.nfields);
  for (uint32_t i = 0; i < a.nfields; ++i) {
    host_dst[i] = a.f[i].dst;
    a.f[i].dst = result + nsignals * MGX_NUM_STATS * a.f[i].col0;
  }
  e = mgx::launch_summary_final(a, p->s_comp);
  for (uint32_t i = 0; i < a.nfields && e == hipSuccess; ++i)
    e = hipMemcpyAsync(host_dst[i], a.f[i].dst, nsignals * MGX_NUM_STATS * a.f[i].width * sizeof(double), hipMemcpyDeviceToHost,
                       p->s_comp);
  if (q.any() && e == hipSuccess) {
    // the operator and the pooling over the whole call's rows, as the device call runs them
    std::vector<double*> delta_dst[2];
    for (int k = 0; k < 2; ++k) {
      mgx::SummaryArgs& da = q.sf[k].a;
      double* const dres = reinterpret_cast<double*>(p->s_delta + dl.result[k]);
      for (uint32_t i = 0; i < da.nfields; ++i) {
        delta_dst[k].push_back(da.f[i].dst);
        da.f[i].dst = dres + nsignals * MGX_NUM_STATS * da.f[i].col0;
      }
    }
    const mgx::Outputs xr = mgx::out_at(p->s_delta, xoff);
    rc = delta_pool(p->d, q, xr, p->s_delta, dl, reinterpret_cast<const uint64_t*>(p->s_delta + dl.table), nframes, nsignals, p->s_comp);
    for (int k = 0; k < 2 && rc == MGX_OK && e == hipSuccess; ++k) {
      const mgx::SummaryArgs& da = q.sf[k].a;
      for (uint32_t i = 0; i < da.nfields && e == hipSuccess; ++i)
        e = hipMemcpyAsync(delta_dst[k][i], da.f[i].dst, nsignals * MGX_NUM_STATS * da.f[i].width * sizeof(double),
                           hipMemcpyDeviceToHost, p->s_comp);
    }
  }
  if (fq.any() && rc == MGX_OK && e == hipSuccess) {
    // the pooling over the whole call's flux columns, as the device call runs it
    mgx::SummaryArgs& fa = fq.sf.a;
    double* const fres = reinterpret_cast<double*>(p->s_flux + fl.result);
    double* flux_dst[MGX_FLUX_MAX_REQUESTS];
    float* col[MGX_FLUX_MAX_REQUESTS];
    for (uint32_t i = 0; i < fq.n; ++i) col[i] = reinterpret_cast<float*>(p->s_flux + fl.col[i]);
    for (uint32_t k = 0; k < fa.nfields; ++k) {
      flux_dst[k] = fa.f[k].dst;
      fa.f[k].dst = fres + nsignals * MGX_NUM_STATS * k;
    }
    rc = flux_pool(fq, col, p->s_flux, fl, reinterpret_cast<const uint64_t*>(p->s_flux + fl.table), nframes, nsignals, p->s_comp);
    for (uint32_t k = 0; k < fa.nfields && rc == MGX_OK && e == hipSuccess; ++k)
      e = hipMemcpyAsync(flux_dst[k], fa.f[k].dst, nsignals * MGX_NUM_STATS * sizeof(double), hipMemcpyDeviceToHost, p->s_comp);
    for (uint32_t i = 0; i < fq.n && rc == MGX_OK && e == hipSuccess; ++i)
      // (the rows of the signals, [frame_offsets[0], frame_offsets[S]): the others are not written, as in the device call)
      if (fq.r[i].per_frame && frame_offsets[nsignals] > frame_offsets[0])
        e = hipMemcpyAsync(fq.r[i].per_frame + frame_offsets[0], col[i] + frame_offsets[0],
                           (frame_offsets[nsignals] - frame_offsets[0]) * sizeof(float), hipMemcpyDeviceToHost, p->s_comp);
    if (pick && rc == MGX_OK && e == hipSuccess) {
      // the picker over the first request's column where it lies, once; the counts and the peaks alone cross back,
      // the peaks when the counts are known (the stream is synchronised below either way)
      mgx_peak_outputs po{};
      po.struct_size = sizeof(po);
      po.peak_offsets = reinterpret_cast<uint64_t*>(p->s_flux + pick_off);
      po.peaks = pick_cap > 0 ? reinterpret_cast<uint64_t*>(p->s_flux + pick_peaks) : nullptr;
      po.capacity = pick_cap;
      e = mgx::launch_peaks(col[0], nframes, false, reinterpret_cast<const uint64_t*>(p->s_flux + fl.table), nsignals, *pick->params,
                            po, p->s_flux + pick_ws, p->s_comp);
      if (e == hipSuccess)
        e = hipMemcpyAsync(pick->peak_offsets, po.peak_offsets, (nsignals + 1) * 8, hipMemcpyDeviceToHost, p->s_comp);
      if (e == hipSuccess) e = hipStreamSynchronize(p->s_comp);
      const uint64_t total = e == hipSuccess ? std::min(pick->peak_offsets[nsignals], pick_cap) : 0;
      if (total > 0) e = hipMemcpyAsync(pick->peaks, po.peaks, total * 8, hipMemcpyDeviceToHost, p->s_comp);
    }
    if (tempo && rc == MGX_OK && e == hipSuccess) {
      // the tempogram of the request's column where it lies, a pass of rows at a time, pooled and picked; the
      // summaries and the lags alone cross back
      const mgx_tempo_params& tp = *tempo->params;
      const TempoLayout tl = tempo_layout(nframes, nsignals, tempo_L, false);
      e = hipMemcpyAsync(p->s_tempo + tempo_win, tempo->window, tp.win_length * sizeof(float), hipMemcpyHostToDevice, p->s_comp);
      if (e == hipSuccess && (tempo->lag || beats))
        e = hipMemcpyAsync(p->s_tempo + tempo_prior, tempo->prior, tp.num_lags * sizeof(double), hipMemcpyHostToDevice, p->s_comp);
      uint32_t* const dlag = tempo->lag || beats ? reinterpret_cast<uint32_t*>(p->s_tempo + tempo_lag) : nullptr;
      if (e == hipSuccess)
        e = tempo_run(col[0], nframes, false, reinterpret_cast<const uint64_t*>(p->s_flux + fl.table), nsignals, tp,
                      reinterpret_cast<const float*>(p->s_tempo + tempo_win), reinterpret_cast<const double*>(p->s_tempo + tempo_prior),
                      nullptr, nullptr, true, dlag, p->s_tempo + tempo_ws, p->s_comp);
      if (e == hipSuccess && tempo->summary)
        e = hipMemcpyAsync(tempo->summary, p->s_tempo + tempo_ws + tl.result, nsignals * MGX_NUM_STATS * tp.num_lags * sizeof(double),
                           hipMemcpyDeviceToHost, p->s_comp);
      if (e == hipSuccess && tempo->lag)
        e = hipMemcpyAsync(tempo->lag, dlag, nsignals * sizeof(uint32_t), hipMemcpyDeviceToHost, p->s_comp);
      if (beats && e == hipSuccess) {
        // the tracker over the same column, the lags where the pick left them as its periods; the counts and the
        // beats alone cross back, the beats when the counts are known
        e = hipMemcpyAsync(p->s_tempo + beat_gauss, beats->gauss, beat_gauss_count(beat_P) * sizeof(float), hipMemcpyHostToDevice, p->s_comp);
        if (e == hipSuccess)
          e = hipMemcpyAsync(p->s_tempo + beat_pen, beats->penalty, beat_penalty_count(beat_P) * sizeof(double), hipMemcpyHostToDevice,
                             p->s_comp);
        mgx_peak_outputs po{};
        po.struct_size = sizeof(po);
        po.peak_offsets = reinterpret_cast<uint64_t*>(p->s_tempo + beat_off);
        po.peaks = beat_cap > 0 ? reinterpret_cast<uint64_t*>(p->s_tempo + beat_rows) : nullptr;
        po.capacity = beat_cap;
        if (e == hipSuccess)
          e = mgx::launch_beats(col[0], nframes, false, reinterpret_cast<const uint64_t*>(p->s_flux + fl.table), nsignals, dlag, beat_P,
                                beats->params->trim, reinterpret_cast<const float*>(p->s_tempo + beat_gauss),
                                reinterpret_cast<const double*>(p->s_tempo + beat_pen), nullptr, nullptr, po, p->s_tempo + beat_ws, p->s_comp);
        if (e == hipSuccess)
          e = hipMemcpyAsync(beats->peak_offsets, po.peak_offsets, (nsignals + 1) * 8, hipMemcpyDeviceToHost, p->s_comp);
        if (e == hipSuccess) e = hipStreamSynchronize(p->s_comp);
        const uint64_t total = e == hipSuccess ? std::min(beats->peak_offsets[nsignals], beat_cap) : 0;
        if (total > 0) e = hipMemcpyAsync(beats->peaks, po.peaks, total * 8, hipMemcpyDeviceToHost, p->s_comp);
      }
    }
  }
  const hipError_t es = hipStreamSynchronize(p->s_comp);
  if (rc) return rc;
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? MGX_OK : hip_fail(e, "summary kernels and copies");
}

}  // namespace

extern "C" {

void mgx_chroma_params_init(mgx_chroma_params* c) {
  if (!c) return;
  memset(c, 0, sizeof *c);
  c->struct_size = sizeof *c;
  c->num_chroma = 12;
  c->a440 = 440.0;
  c->center_octave = 5.0;
  c->octave_width = 2.0;
  c->base_c = 1;
}

// The construction of librosa.filters.chroma as include/meyda_gpu.h states it: float64 throughout, one rounding
int mgx_chroma_weights(uint32_t buffer_size, double sample_rate, const mgx_chroma_params* c, float* weights) {
  if (!c) return fail(MGX_E_INVALID_ARGUMENT, "params is NULL");
  if (c->struct_size != sizeof(mgx_chroma_params))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_params.struct_size is %u, expected %zu", c->struct_size, sizeof(mgx_chroma_params));
  if (!weights) return fail(MGX_E_INVALID_ARGUMENT, "weights is NULL");
  if (c->num_chroma < 1 || c->num_chroma > MGX_CHROMA_MAX_BINS)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_params.num_chroma is %u, expected 1..%d", c->num_chroma, MGX_CHROMA_MAX_BINS);
  if (!(std::isfinite(sample_rate) && sample_rate > 0)) return fail(MGX_E_INVALID_ARGUMENT, "sample_rate must be finite and positive");
  if (!(std::isfinite(c->a440) && c->a440 > 0)) return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_params.a440 must be finite and positive");
  if (!(std::isfinite(c->octave_width) && c->octave_width >= 0))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_params.octave_width must be finite and not negative");
  if (!std::isfinite(c->center_octave)) return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_params.center_octave must be finite");
  if (buffer_size < 4 || (buffer_size & (buffer_size - 1)) != 0)
    return fail(MGX_E_NOT_POWER_OF_TWO, "Buffer size is not a power of two of at least 4: %u", buffer_size);
  const uint32_t C = c->num_chroma, K = buffer_size / 2;
  const double Cd = (double)C, n = (double)buffer_size;
  std::vector<double> fb((size_t)K + 1);
  for (uint32_t k = 1; k <= K; ++k) fb[k] = Cd * std::log2(((double)k * sample_rate / n) / (c->a440 / 16.0));
  fb[0] = fb[1] - 1.5 * Cd;
  const double h = std::nearbyint(Cd / 2.0);  // (the default rounding mode: ties to even)
  const uint32_t roll = c->base_c ? 3 * (C / 12) : 0;
  std::vector<double> col(C);
  for (uint32_t k = 0; k < K; ++k) {
    const double bw = std::max(fb[k + 1] - fb[k], 1.0);
    double ss = 0.0;
    for (uint32_t i = 0; i < C; ++i) {
      double m = std::fmod(fb[k] - (double)i + h, Cd);  // exact; the sign of the dividend
      if (m < 0) m += Cd;
      const double d = m - h, t = 2.0 * d / bw;
      col[i] = std::exp(-0.5 * (t * t));
      ss += col[i] * col[i];
    }
    const double norm = std::sqrt(ss);
    double oct = 1.0;
    if (c->octave_width > 0) {
      const double u = (fb[k] / Cd - c->center_octave) / c->octave_width;
      oct = std::exp(-0.5 * (u * u));
    }
    for (uint32_t i = 0; i < C; ++i) {
      double v = col[(i + roll) % C] / norm;
      if (c->octave_width > 0) v *= oct;
      // the one rounding; a positive value below the smallest float32 takes that value instead of +0, so the table
      // stays strictly positive as it is in float64 (a zero weight would turn an overflowed amplitude into NaN)
      const float f = (float)v;
      weights[(size_t)i * K + k] = v > 0.0 && f == 0.0f ? std::numeric_limits<float>::denorm_min() : f;
    }
  }
  return MGX_OK;
}

int mgx_chroma_device(const float* rows, uint64_t num_frames, uint32_t cols, const float* weights, uint32_t num_chroma, uint32_t norm,
                      float* chroma, void* stream) {
  if (cols == 0) return fail(MGX_E_INVALID_ARGUMENT, "cols is 0");
  if (num_chroma < 1 || num_chroma > MGX_CHROMA_MAX_BINS)
    return fail(MGX_E_INVALID_ARGUMENT, "num_chroma is %u, expected 1..%d", num_chroma, MGX_CHROMA_MAX_BINS);
  if (norm >= MGX_NUM_CHROMA_NORMS) return fail(MGX_E_INVALID_ARGUMENT, "norm is %u, expected 0..%d", norm, MGX_NUM_CHROMA_NORMS - 1);
  if (!weights) return fail(MGX_E_INVALID_ARGUMENT, "weights is NULL");
  if (!chroma) return fail(MGX_E_INVALID_ARGUMENT, "chroma is NULL");
  if (chroma == rows || chroma == weights) return fail(MGX_E_INVALID_ARGUMENT, "chroma is the same array as %s", chroma == rows ? "rows" : "weights");
  if (num_frames > 0 && !rows) return fail(MGX_E_INVALID_ARGUMENT, "rows is NULL");
  if (num_frames == 0) return MGX_OK;
  const hipError_t e = mgx::launch_chroma(rows, num_frames, cols, weights, num_chroma, norm, chroma, (hipStream_t)stream);
  return e == hipSuccess ? MGX_OK : hip_fail(e, "chroma kernel launch");
}

int mgx_chroma_host(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                    const uint64_t* frame_offsets, uint64_t nsignals, const mgx_chroma_request* req) {
  if (!req) return fail(MGX_E_INVALID_ARGUMENT, "request is NULL");
  if (req->struct_size != sizeof(mgx_chroma_request))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.struct_size is %u, expected %zu", req->struct_size, sizeof(mgx_chroma_request));
  if (req->num_chroma < 1 || req->num_chroma > MGX_CHROMA_MAX_BINS)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.num_chroma is %u, expected 1..%d", req->num_chroma, MGX_CHROMA_MAX_BINS);
  if (req->norm >= MGX_NUM_CHROMA_NORMS)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.norm is %u, expected 0..%d", req->norm, MGX_NUM_CHROMA_NORMS - 1);
  if (!req->weights) return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.weights is NULL");
  if (!req->per_frame && !req->summary) return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.per_frame and .summary are both NULL");
  if (req->summary && nsignals == 0) return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.summary is set with num_signals = 0");
  if (!p) return fail(MGX_E_INVALID_ARGUMENT, "plan is NULL");
  int rc = summary_inputs(p, samples, num_samples, starts, nframes, frame_offsets, nsignals);
  if (rc) return rc;
  // (the host sees both tables: they are checked here, before any copy, as mgx_summarize_host checks them)
  const uint64_t n = (uint64_t)p->n;
  for (uint64_t f = 0; f < nframes; ++f)
    if (starts[f] > num_samples - n)
      return fail(MGX_E_INVALID_ARGUMENT, "starts[%llu] = %llu: a buffer of %d leaves the %llu samples", (unsigned long long)f,
                  (unsigned long long)starts[f], p->n, (unsigned long long)num_samples);
  for (uint64_t s = 0; s < nsignals; ++s)
    if (frame_offsets[s + 1] < frame_offsets[s])
      return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets[%llu] = %llu is below frame_offsets[%llu] = %llu", (unsigned long long)(s + 1),
                  (unsigned long long)frame_offsets[s + 1], (unsigned long long)s, (unsigned long long)frame_offsets[s]);
  if (nsignals > 0 && frame_offsets[nsignals] > nframes)
    return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets[%llu] = %llu is above the %llu buffers", (unsigned long long)nsignals,
                (unsigned long long)frame_offsets[nsignals], (unsigned long long)nframes);
  const mgx_outputs none{};
  mgx::Outputs x;  // (no per-frame field crosses back)
  if ((rc = make_outputs(p, &none, nullptr, &x))) return rc;
  resident_stop(p);
  const uint32_t C = req->num_chroma, cols = (uint32_t)(n / 2);
  const uint64_t stats = nsignals * MGX_NUM_STATS * C;
  if (nframes == 0) {
    // no buffers: every signal is empty, NaN in all four (nothing for the device to do)
    if (req->summary) std::fill_n(req->summary, stats, std::nan(""));
    return MGX_OK;
  }
  // the call's buffer: the bank, the chroma rows, and for the pooling a table, the shifts, the partials and the summaries
  const bool pool = req->summary != nullptr;
  uint64_t total = 0;
  auto take = [&total](uint64_t bytes) {
    const uint64_t at = total;
    total += (bytes + 255) / 256 * 256;
    return at;
  };
  const uint64_t at_bank = take((uint64_t)C * cols * sizeof(float)), at_rows = take(nframes * C * sizeof(float));
  const uint64_t at_table = pool ? take((nsignals + 1) * sizeof(uint64_t)) : 0, at_shift = pool ? take(nsignals * C * sizeof(double)) : 0;
  const uint64_t at_part = pool ? take((nframes / mgx::kSummaryBlock + nsignals + 1) * mgx::kSummaryWords * C * sizeof(double)) : 0;
  const uint64_t at_result = pool ? take(stats * sizeof(double)) : 0;
  hipError_t e = hipSetDevice(p->d.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  // the staging streams first: the bank's copy and the last kernels go on the compute stream
  if ((rc = ensure_host_staging(p, 1, mgx::kOutLayoutSlack))) return rc;
  if (p->s_chroma_bytes < total) {
    if (p->s_chroma) (void)hipFree(p->s_chroma);
    p->s_chroma = nullptr;
    p->s_chroma_bytes = 0;
    e = hipMalloc(reinterpret_cast<void**>(&p->s_chroma), total);
    if (e != hipSuccess) { p->s_chroma = nullptr; return hip_fail(e, "hipMalloc(chroma rows)"); }
    p->s_chroma_bytes = total;
  }
  const float* const bank = reinterpret_cast<const float*>(p->s_chroma + at_bank);
  float* const out = reinterpret_cast<float*>(p->s_chroma + at_rows);
  e = hipMemcpyAsync(p->s_chroma + at_bank, req->weights, (uint64_t)C * cols * sizeof(float), hipMemcpyHostToDevice, p->s_comp);
  if (e == hipSuccess && pool)
    e = hipMemcpyAsync(p->s_chroma + at_table, frame_offsets, (nsignals + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p->s_comp);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(p->s_comp);
    return hip_fail(e, "hipMemcpyAsync(weights, frame_offsets)");
  }
  ChunkHook hook;
  hook.pooled = MGX_OUT_AMPLITUDE_SPECTRUM;
  hook.after = [&](uint64_t f0, uint64_t cnt, const mgx::Outputs& d) {
    const hipError_t ke = mgx::launch_chroma(d.amplitude_spectrum, cnt, cols, bank, C, req->norm, out + f0 * C, p->s_comp);
    return ke == hipSuccess ? (int)MGX_OK : hip_fail(ke, "chroma kernel launch");
  };
  if ((rc = gather_host_chunked(p, samples, starts, nframes, &x, &hook))) return rc;
  if (req->per_frame) e = hipMemcpyAsync(req->per_frame, out, nframes * C * sizeof(float), hipMemcpyDeviceToHost, p->s_comp);
  if (pool && e == hipSuccess) {
    // the summary kernels over the whole call's chroma rows: one field of width C, keyed by the table
    mgx::SummaryArgs a{};
    a.nfields = 1;
    a.cols = C;
    a.f[0].src = out;
    a.f[0].dst = reinterpret_cast<double*>(p->s_chroma + at_result);
    a.f[0].width = C;
    a.table = reinterpret_cast<const uint64_t*>(p->s_chroma + at_table);
    a.num_signals = nsignals;
    a.num_frames = nframes;
    a.rows = nframes;
    a.nslots = nframes / mgx::kSummaryBlock + nsignals;
    a.shift = reinterpret_cast<double*>(p->s_chroma + at_shift);
    a.part = reinterpret_cast<double*>(p->s_chroma + at_part);
    e = mgx::launch_summary_partial(a, p->s_comp);
    if (e == hipSuccess) e = mgx::launch_summary_final(a, p->s_comp);
    if (e == hipSuccess) e = hipMemcpyAsync(req->summary, a.f[0].dst, stats * sizeof(double), hipMemcpyDeviceToHost, p->s_comp);
  }
  const hipError_t es = hipStreamSynchronize(p->s_comp);
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? MGX_OK : hip_fail(e, "chroma and summary kernels and copies");
}

void mgx_hpss_params_init(mgx_hpss_params* h) {
  if (!h) return;
  memset(h, 0, sizeof *h);
  h->struct_size = sizeof *h;
  h->kernel_time = MGX_HPSS_MAX_KERNEL;
  h->kernel_freq = MGX_HPSS_MAX_KERNEL;
  h->mode = MGX_HPSS_SOFT2;
  h->margin_harmonic = 1.0f;
  h->margin_percussive = 1.0f;
}

void mgx_hpss_tile(uint32_t* tile_rows, uint32_t* tile_cols) {
  if (tile_rows) *tile_rows = MGX_HPSS_TILE_ROWS;
  if (tile_cols) *tile_cols = MGX_HPSS_TILE_COLS;
}

static int check_hpss_params(const mgx_hpss_params* hp) {
  if (!hp) return fail(MGX_E_INVALID_ARGUMENT, "params is NULL");
  if (hp->struct_size != sizeof(mgx_hpss_params))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_hpss_params.struct_size is %u, expected %zu", hp->struct_size, sizeof(mgx_hpss_params));
  const uint32_t k[2] = {hp->kernel_time, hp->kernel_freq};
  for (int i = 0; i < 2; ++i)
    if (!(k[i] & 1u) || k[i] > MGX_HPSS_MAX_KERNEL)
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_hpss_params.kernel_%s is %u, expected an odd value in 1..%d", i ? "freq" : "time", k[i],
                  MGX_HPSS_MAX_KERNEL);
  if (hp->mode >= MGX_NUM_HPSS_MODES)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_hpss_params.mode is %u, expected 0..%d", hp->mode, MGX_NUM_HPSS_MODES - 1);
  const float m[2] = {hp->margin_harmonic, hp->margin_percussive};
  for (int i = 0; i < 2; ++i)
    if (!std::isfinite(m[i]) || !(m[i] >= 1.0f))
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_hpss_params.margin_%s is %g, expected a finite value >= 1", i ? "percussive" : "harmonic",
                  (double)m[i]);
  return MGX_OK;
}

int mgx_hpss_device(const float* rows, uint64_t num_frames, uint32_t cols, const uint64_t* frame_offsets, uint64_t num_signals,
                    const mgx_hpss_params* params, float* harmonic, float* percussive, void* stream) {
  const int rc = check_hpss_params(params);
  if (rc) return rc;
  if (cols == 0) return fail(MGX_E_INVALID_ARGUMENT, "cols is 0");
  if (!harmonic && !percussive) return fail(MGX_E_INVALID_ARGUMENT, "harmonic and percussive are both NULL");
  if (harmonic == percussive) return fail(MGX_E_INVALID_ARGUMENT, "harmonic and percussive are the same array");
  if (rows && (harmonic == rows || percussive == rows)) return fail(MGX_E_INVALID_ARGUMENT, "an output is the rows' own array");
  if (num_signals > 0 && !frame_offsets) return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets is NULL");
  if (num_frames == 0) return MGX_OK;
  if (!rows) return fail(MGX_E_INVALID_ARGUMENT, "rows is NULL");
  // (frame_offsets with num_signals = 0: a table of one entry, no signal, nothing written)
  const hipError_t e = mgx::launch_hpss(rows, num_frames, cols, frame_offsets, num_signals, *params, harmonic, percussive, (hipStream_t)stream);
  return e == hipSuccess ? MGX_OK : hip_fail(e, "hpss kernel launch");
}

int mgx_hpss_host(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                  const uint64_t* frame_offsets, uint64_t nsignals, const mgx_hpss_params* params, const mgx_chroma_request* chroma,
                  const mgx_flux_request* flux, float* harmonic, float* percussive) {
  int rc = check_hpss_params(params);
  if (rc) return rc;
  if (!chroma && !flux && !harmonic && !percussive)
    return fail(MGX_E_INVALID_ARGUMENT, "harmonic_chroma, percussive_flux, harmonic and percussive are all NULL");
  if (harmonic && harmonic == percussive) return fail(MGX_E_INVALID_ARGUMENT, "harmonic and percussive are the same array");
  if (chroma) {
    if (chroma->struct_size != sizeof(mgx_chroma_request))
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.struct_size is %u, expected %zu", chroma->struct_size, sizeof(mgx_chroma_request));
    if (chroma->num_chroma < 1 || chroma->num_chroma > MGX_CHROMA_MAX_BINS)
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.num_chroma is %u, expected 1..%d", chroma->num_chroma, MGX_CHROMA_MAX_BINS);
    if (chroma->norm >= MGX_NUM_CHROMA_NORMS)
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.norm is %u, expected 0..%d", chroma->norm, MGX_NUM_CHROMA_NORMS - 1);
    if (!chroma->weights) return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.weights is NULL");
    if (!chroma->per_frame && !chroma->summary)
      return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.per_frame and .summary are both NULL");
    if (chroma->summary && nsignals == 0) return fail(MGX_E_INVALID_ARGUMENT, "mgx_chroma_request.summary is set with num_signals = 0");
  }
  FluxReq fq;
  if (flux) {
    if ((rc = flux_request(nullptr, flux, 1, nsignals, &fq))) return rc;
    if (flux->field != MGX_AMPLITUDE_SPECTRUM)
      return fail(MGX_E_UNSUPPORTED, "mgx_flux_request.field is %u: the percussive rows are amplitude rows (MGX_AMPLITUDE_SPECTRUM)", flux->field);
  }
  if (!p) return fail(MGX_E_INVALID_ARGUMENT, "plan is NULL");
  if ((rc = summary_inputs(p, samples, num_samples, starts, nframes, frame_offsets, nsignals))) return rc;
  // (the host sees both tables: they are checked here, before any copy, as mgx_chroma_host checks them)
  const uint64_t n = (uint64_t)p->n;
  for (uint64_t f = 0; f < nframes; ++f)
    if (starts[f] > num_samples - n)
      return fail(MGX_E_INVALID_ARGUMENT, "starts[%llu] = %llu: a buffer of %d leaves the %llu samples", (unsigned long long)f,
                  (unsigned long long)starts[f], p->n, (unsigned long long)num_samples);
  for (uint64_t s = 0; s < nsignals; ++s)
    if (frame_offsets[s + 1] < frame_offsets[s])
      return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets[%llu] = %llu is below frame_offsets[%llu] = %llu", (unsigned long long)(s + 1),
                  (unsigned long long)frame_offsets[s + 1], (unsigned long long)s, (unsigned long long)frame_offsets[s]);
  if (nsignals > 0 && frame_offsets[nsignals] > nframes)
    return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets[%llu] = %llu is above the %llu buffers", (unsigned long long)nsignals,
                (unsigned long long)frame_offsets[nsignals], (unsigned long long)nframes);
  const mgx_outputs none{};
  mgx::Outputs x;  // (no per-frame field crosses back)
  if ((rc = make_outputs(p, &none, nullptr, &x))) return rc;
  resident_stop(p);
  const uint32_t cols = (uint32_t)(n / 2), C = chroma ? chroma->num_chroma : 0;
  const uint64_t cstats = nsignals * MGX_NUM_STATS * C, fstats = nsignals * MGX_NUM_STATS;
  if (nframes == 0) {
    // no buffers: every signal is empty, NaN in all four (nothing for the device to do)
    if (chroma && chroma->summary) std::fill_n(chroma->summary, cstats, std::nan(""));
    if (flux && flux->summary) std::fill_n(flux->summary, fstats, std::nan(""));
    return MGX_OK;
  }
  // the rows the operator writes and the copies back cover: the signals' own, or every row without a table
  const bool has_table = frame_offsets != nullptr;
  const uint64_t w0 = has_table ? (nsignals ? std::min(frame_offsets[0], nframes) : 0) : 0;
  const uint64_t w1 = has_table ? (nsignals ? std::min(frame_offsets[nsignals], nframes) : 0) : nframes;
  const bool need_h = harmonic || chroma, need_p = percussive || flux;
  const bool cpool = chroma && chroma->summary, fpool = flux && flux->summary;
  const uint64_t parts = nframes / mgx::kSummaryBlock + nsignals + 1;
  uint64_t total = 0;
  auto take = [&total](uint64_t bytes) {
    const uint64_t at = total;
    total += (bytes + 255) / 256 * 256;
    return at;
  };
  const uint64_t row_bytes = nframes * cols * sizeof(float);
  const uint64_t at_amp = take(row_bytes), at_h = need_h ? take(row_bytes) : 0, at_p = need_p ? take(row_bytes) : 0;
  const uint64_t at_table = has_table ? take((nsignals + 1) * sizeof(uint64_t)) : 0;
  const uint64_t at_bank = chroma ? take((uint64_t)C * cols * sizeof(float)) : 0, at_crows = chroma ? take(nframes * C * sizeof(float)) : 0;
  const uint64_t at_cshift = cpool ? take(nsignals * C * sizeof(double)) : 0;
  const uint64_t at_cpart = cpool ? take(parts * mgx::kSummaryWords * C * sizeof(double)) : 0, at_cres = cpool ? take(cstats * sizeof(double)) : 0;
  const uint64_t at_fcol = flux ? take(nframes * sizeof(float)) : 0, at_fshift = fpool ? take(nsignals * sizeof(double)) : 0;
  const uint64_t at_fpart = fpool ? take(parts * mgx::kSummaryWords * sizeof(double)) : 0, at_fres = fpool ? take(fstats * sizeof(double)) : 0;
  hipError_t e = hipSetDevice(p->d.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  if ((rc = ensure_host_staging(p, 1, mgx::kOutLayoutSlack))) return rc;
  if (p->s_hpss_bytes < total) {
    if (p->s_hpss) (void)hipFree(p->s_hpss);
    p->s_hpss = nullptr;
    p->s_hpss_bytes = 0;
    e = hipMalloc(reinterpret_cast<void**>(&p->s_hpss), total);
    if (e != hipSuccess) {
      p->s_hpss = nullptr;
      return hip_fail(e, "hipMalloc(hpss rows)");  // (MGX_E_OUT_OF_MEMORY when the device has no room)
    }
    p->s_hpss_bytes = total;
  }
  unsigned char* const buf = p->s_hpss;
  float* const amp = reinterpret_cast<float*>(buf + at_amp);
  float* const dh = need_h ? reinterpret_cast<float*>(buf + at_h) : nullptr;
  float* const dp = need_p ? reinterpret_cast<float*>(buf + at_p) : nullptr;
  const uint64_t* const table = has_table ? reinterpret_cast<const uint64_t*>(buf + at_table) : nullptr;
  if (has_table) e = hipMemcpyAsync(buf + at_table, frame_offsets, (nsignals + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p->s_comp);
  if (e == hipSuccess && chroma)
    e = hipMemcpyAsync(buf + at_bank, chroma->weights, (uint64_t)C * cols * sizeof(float), hipMemcpyHostToDevice, p->s_comp);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(p->s_comp);
    return hip_fail(e, "hipMemcpyAsync(frame_offsets, weights)");
  }
  ChunkHook hook;
  hook.pooled = MGX_OUT_AMPLITUDE_SPECTRUM;
  hook.after = [&](uint64_t f0, uint64_t cnt, const mgx::Outputs& d) {
    // the chunk's amplitude rows into the call's array before the slot is reused
    const hipError_t ke =
        hipMemcpyAsync(amp + f0 * cols, d.amplitude_spectrum, cnt * cols * sizeof(float), hipMemcpyDeviceToDevice, p->s_comp);
    return ke == hipSuccess ? (int)MGX_OK : hip_fail(ke, "hipMemcpyAsync(amplitude rows)");
  };
  if ((rc = gather_host_chunked(p, samples, starts, nframes, &x, &hook))) return rc;
  hipStream_t st = p->s_comp;
  e = mgx::launch_hpss(amp, nframes, cols, table, nsignals, *params, dh, dp, st);
  const uint64_t wn = w1 > w0 ? w1 - w0 : 0;
  if (e == hipSuccess && harmonic && wn)
    e = hipMemcpyAsync(harmonic + w0 * cols, dh + w0 * cols, wn * cols * sizeof(float), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && percussive && wn)
    e = hipMemcpyAsync(percussive + w0 * cols, dp + w0 * cols, wn * cols * sizeof(float), hipMemcpyDeviceToHost, st);
  auto pool = [&](const float* src, uint32_t width, uint64_t at_shift, uint64_t at_part, uint64_t at_res, double* dst, uint64_t count) {
    mgx::SummaryArgs a{};
    a.nfields = 1;
    a.cols = width;
    a.f[0].src = src;
    a.f[0].dst = reinterpret_cast<double*>(buf + at_res);
    a.f[0].width = width;
    a.table = table;
    a.num_signals = nsignals;
    a.num_frames = nframes;
    a.rows = nframes;
    a.nslots = nframes / mgx::kSummaryBlock + nsignals;
    a.shift = reinterpret_cast<double*>(buf + at_shift);
    a.part = reinterpret_cast<double*>(buf + at_part);
    hipError_t pe = mgx::launch_summary_partial(a, st);
    if (pe == hipSuccess) pe = mgx::launch_summary_final(a, st);
    if (pe == hipSuccess) pe = hipMemcpyAsync(dst, a.f[0].dst, count * sizeof(double), hipMemcpyDeviceToHost, st);
    return pe;
  };
  if (e == hipSuccess && chroma && wn) {
    // chroma of the harmonic rows of the signals (a row of no signal holds nothing the operator wrote)
    float* const crows = reinterpret_cast<float*>(buf + at_crows);
    e = mgx::launch_chroma(dh + w0 * cols, wn, cols, reinterpret_cast<const float*>(buf + at_bank), C, chroma->norm, crows + w0 * C, st);
    if (e == hipSuccess && chroma->per_frame)
      e = hipMemcpyAsync(chroma->per_frame + w0 * C, crows + w0 * C, wn * C * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && cpool) e = pool(crows, C, at_cshift, at_cpart, at_cres, chroma->summary, cstats);
  } else if (e == hipSuccess && cpool) {
    std::fill_n(chroma->summary, cstats, std::nan(""));
  }
  if (e == hipSuccess && flux && wn) {
    float* const fcol = reinterpret_cast<float*>(buf + at_fcol);
    e = mgx::launch_flux(dp, nullptr, fcol, 0, nframes, nframes, cols, false, table, nsignals, flux->mode, flux->lag, st);
    if (e == hipSuccess && flux->per_frame)
      e = hipMemcpyAsync(flux->per_frame + w0, fcol + w0, wn * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && fpool) e = pool(fcol, 1, at_fshift, at_fpart, at_fres, flux->summary, fstats);
  } else if (e == hipSuccess && fpool) {
    std::fill_n(flux->summary, fstats, std::nan(""));
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? MGX_OK : hip_fail(e, "hpss, chroma, flux and summary kernels and copies");
}

void mgx_tempo_params_init(mgx_tempo_params* t) {
  if (!t) return;
  memset(t, 0, sizeof *t);
  t->struct_size = sizeof *t;
  t->win_length = 384;
  t->num_lags = 384;
  t->norm = MGX_TEMPOGRAM_NORM_LAG0;
  t->gain = 1e6;
}

int mgx_tempogram_window(uint32_t W, float* h) {
  if (W < 2 || W > MGX_TEMPOGRAM_MAX_WIN) return fail(MGX_E_INVALID_ARGUMENT, "win_length is %u, expected 2..%d", W, MGX_TEMPOGRAM_MAX_WIN);
  if (!h) return fail(MGX_E_INVALID_ARGUMENT, "window is NULL");
  const double two_pi = 6.283185307179586476925286766559;
  for (uint32_t j = 0; j < W; ++j) h[j] = (float)(0.5 - 0.5 * std::cos(two_pi * (double)j / (double)W));
  return MGX_OK;
}

int mgx_tempo_prior(double frame_rate, double start_bpm, double std_octaves, double max_bpm, uint32_t L, double* prior) {
  if (!(std::isfinite(frame_rate) && frame_rate > 0)) return fail(MGX_E_INVALID_ARGUMENT, "frame_rate must be finite and positive");
  if (!(std::isfinite(start_bpm) && start_bpm > 0)) return fail(MGX_E_INVALID_ARGUMENT, "start_bpm must be finite and positive");
  if (!(std::isfinite(std_octaves) && std_octaves > 0)) return fail(MGX_E_INVALID_ARGUMENT, "std_octaves must be finite and positive");
  if (!(max_bpm >= 0)) return fail(MGX_E_INVALID_ARGUMENT, "max_bpm must not be negative or NaN (0: no limit)");
  if (L == 0) return fail(MGX_E_INVALID_ARGUMENT, "num_lags is 0");
  if (!prior) return fail(MGX_E_INVALID_ARGUMENT, "prior is NULL");
  prior[0] = 0.0;
  const double l2s = std::log2(start_bpm);
  for (uint32_t l = 1; l < L; ++l) {
    const double bpm = 60.0 * frame_rate / (double)l;
    if (max_bpm > 0 && bpm > max_bpm) {
      prior[l] = 0.0;
      continue;
    }
    const double z = (std::log2(bpm) - l2s) / std_octaves;
    prior[l] = std::exp(-0.5 * (z * z));
  }
  return MGX_OK;
}

// what mgx_tempogram_device and mgx_tempo_device refuse about the arguments they share
static int check_tempogram_args(const void* envelope, uint64_t num_frames, uint32_t envelope_f64, const uint64_t* frame_offsets,
                                uint64_t num_signals, const float* window, uint32_t W, uint32_t L, uint32_t norm) {
  if (envelope_f64 > 1) return fail(MGX_E_INVALID_ARGUMENT, "envelope_f64 is %u, expected 0 or 1", envelope_f64);
  if (W < 2 || W > MGX_TEMPOGRAM_MAX_WIN) return fail(MGX_E_INVALID_ARGUMENT, "win_length is %u, expected 2..%d", W, MGX_TEMPOGRAM_MAX_WIN);
  if (L < 1 || L > W) return fail(MGX_E_INVALID_ARGUMENT, "num_lags is %u, expected 1..%u (win_length)", L, W);
  if (norm >= MGX_NUM_TEMPOGRAM_NORMS) return fail(MGX_E_INVALID_ARGUMENT, "norm is %u, expected 0..%d", norm, MGX_NUM_TEMPOGRAM_NORMS - 1);
  if (!window) return fail(MGX_E_INVALID_ARGUMENT, "window is NULL");
  if (num_signals > 0 && !frame_offsets) return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets is NULL");
  if (num_frames > 0 && !envelope) return fail(MGX_E_INVALID_ARGUMENT, "envelope is NULL");
  return MGX_OK;
}

int mgx_tempogram_device(const void* envelope, uint64_t num_frames, uint32_t envelope_f64, const uint64_t* frame_offsets,
                         uint64_t num_signals, const float* window, uint32_t W, uint32_t L, uint32_t norm, float* tempogram,
                         void* stream) {
  const int rc = check_tempogram_args(envelope, num_frames, envelope_f64, frame_offsets, num_signals, window, W, L, norm);
  if (rc) return rc;
  if (!tempogram) return fail(MGX_E_INVALID_ARGUMENT, "tempogram is NULL");
  if (tempogram == envelope || tempogram == window)
    return fail(MGX_E_INVALID_ARGUMENT, "tempogram is the same array as %s", tempogram == envelope ? "envelope" : "window");
  if (num_frames == 0 || (frame_offsets && num_signals == 0)) return MGX_OK;
  const hipError_t e = mgx::launch_tempogram(envelope, num_frames, envelope_f64 != 0, frame_offsets, num_signals, window, W, L, norm,
                                             tempogram, 0, num_frames, (hipStream_t)stream);
  return e == hipSuccess ? MGX_OK : hip_fail(e, "tempogram kernel launch");
}

int mgx_tempo_workspace_bytes(uint64_t num_frames, uint64_t num_signals, const mgx_tempo_params* params, uint32_t keep_rows,
                              uint64_t* bytes) {
  const int rc = check_tempo_params(params);
  if (rc) return rc;
  if (keep_rows > 1) return fail(MGX_E_INVALID_ARGUMENT, "keep_rows is %u, expected 0 or 1", keep_rows);
  if (!bytes) return fail(MGX_E_INVALID_ARGUMENT, "bytes is NULL");
  *bytes = tempo_layout(num_frames, num_signals ? num_signals : 1, params->num_lags, keep_rows != 0).total;
  return MGX_OK;
}

int mgx_tempo_device(const void* envelope, uint64_t num_frames, uint32_t envelope_f64, const uint64_t* frame_offsets,
                     uint64_t num_signals, const mgx_tempo_params* params, const float* window, const double* prior, float* tempogram,
                     double* summary, uint32_t* lag, void* workspace, uint64_t workspace_bytes, void* stream) {
  int rc = check_tempo_params(params);
  if (rc || (rc = check_tempogram_args(envelope, num_frames, envelope_f64, frame_offsets, num_signals, window, params->win_length,
                                       params->num_lags, params->norm)))
    return rc;
  if (!tempogram && !summary && !lag) return fail(MGX_E_INVALID_ARGUMENT, "tempogram, summary and lag are all NULL");
  if (lag && !prior) return fail(MGX_E_INVALID_ARGUMENT, "lag is set without prior");
  if (tempogram && (tempogram == envelope || tempogram == window))
    return fail(MGX_E_INVALID_ARGUMENT, "tempogram is the same array as %s", tempogram == envelope ? "envelope" : "window");
  const uint64_t S = frame_offsets ? num_signals : 1;
  const uint64_t need = tempo_layout(num_frames, S ? S : 1, params->num_lags, tempogram != nullptr).total;
  if (workspace_bytes < need || !workspace)
    return fail(MGX_E_INVALID_ARGUMENT, "the workspace holds %llu bytes, the call needs %llu (mgx_tempo_workspace_bytes)",
                (unsigned long long)(workspace ? workspace_bytes : 0), (unsigned long long)need);
  if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return fail(MGX_E_INVALID_ARGUMENT, "the workspace is not 256-byte aligned");
  if (S == 0) return MGX_OK;  // (a table of no signals: no row, no summary, no lag)
  const hipError_t e = tempo_run(envelope, num_frames, envelope_f64 != 0, frame_offsets, S, *params, window, prior, tempogram, summary,
                                 summary || lag, lag, static_cast<unsigned char*>(workspace), (hipStream_t)stream);
  return e == hipSuccess ? MGX_OK : hip_fail(e, "tempo kernel launch");
}

int mgx_tempo_host(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                   const uint64_t* frame_offsets, uint64_t nsignals, const mgx_flux_request* flux, const mgx_tempo_params* params,
                   const float* window, const double* prior, double* summary, uint32_t* lag) {
  const int rc = check_tempo_params(params);
  if (rc) return rc;
  if (nsignals == 0) return fail(MGX_E_INVALID_ARGUMENT, "num_signals is 0: a tempo is a clip's");
  if (!flux) return fail(MGX_E_INVALID_ARGUMENT, "flux is NULL");
  if (!window) return fail(MGX_E_INVALID_ARGUMENT, "window is NULL");
  if (!summary && !lag) return fail(MGX_E_INVALID_ARGUMENT, "summary and lag are both NULL");
  if (lag && !prior) return fail(MGX_E_INVALID_ARGUMENT, "lag is set without prior");
  mgx_summary_outputs none{};
  none.struct_size = sizeof(none);
  const TempoHost th{params, window, prior, summary, lag, nullptr};
  return summarize_host_impl(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, nullptr, nullptr, &none, nullptr, flux, 1,
                             nullptr, &th);
}

void mgx_beat_params_init(mgx_beat_params* b) {
  if (!b) return;
  memset(b, 0, sizeof *b);
  b->struct_size = sizeof *b;
  b->max_period = MGX_BEAT_MAX_PERIOD;
  b->trim = 1;
}

int mgx_beat_tables(uint32_t P, double tightness, float* gauss, double* penalty) {
  if (P < 1 || P > MGX_BEAT_MAX_PERIOD) return fail(MGX_E_INVALID_ARGUMENT, "max_period is %u, expected 1..%d", P, MGX_BEAT_MAX_PERIOD);
  if (!(std::isfinite(tightness) && tightness > 0)) return fail(MGX_E_INVALID_ARGUMENT, "tightness must be finite and positive");
  if (!gauss) return fail(MGX_E_INVALID_ARGUMENT, "gauss is NULL");
  if (!penalty) return fail(MGX_E_INVALID_ARGUMENT, "penalty is NULL");
  const double ninf = -std::numeric_limits<double>::infinity();
  gauss[0] = 1.0f;
  penalty[0] = ninf;
  for (uint32_t p = 1; p <= P; ++p) {
    float* const g = gauss + (size_t)p * (p + 1) / 2;
    for (uint32_t k = 0; k <= p; ++k) {
      const double z = 32.0 * (double)k / (double)p;
      g[k] = (float)std::exp(-0.5 * (z * z));
    }
    uint32_t lo = p / 2;
    if (p & 1) lo += lo & 1;
    lo = std::max(lo, 1u);
    double* const w = penalty + (size_t)p * p;
    for (uint32_t d = 0; d <= 2 * p; ++d) {
      if (d < lo) {
        w[d] = ninf;
        continue;
      }
      const double l = std::log((double)d / (double)p);
      w[d] = -tightness * (l * l);
    }
  }
  return MGX_OK;
}

int mgx_beats_workspace_bytes(uint64_t num_frames, uint64_t num_signals, uint64_t* bytes) {
  if (!bytes) return fail(MGX_E_INVALID_ARGUMENT, "bytes is NULL");
  *bytes = mgx::beats_workspace_bytes(num_frames, num_signals);
  return MGX_OK;
}

int mgx_beats_device(const void* envelope, uint64_t num_frames, uint32_t envelope_f64, const uint64_t* frame_offsets,
                     uint64_t num_signals, const uint32_t* period, const mgx_beat_params* params, const float* gauss,
                     const double* penalty, double* local_score, double* cum_score, const mgx_peak_outputs* out, void* workspace,
                     uint64_t workspace_bytes, void* stream) {
  const int rc = check_beat_params(params);
  if (rc) return rc;
  if (!out) return fail(MGX_E_INVALID_ARGUMENT, "out is NULL");
  if (out->struct_size != sizeof(mgx_peak_outputs))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.struct_size is %u, expected %zu", out->struct_size, sizeof(mgx_peak_outputs));
  if (envelope_f64 > 1) return fail(MGX_E_INVALID_ARGUMENT, "envelope_f64 is %u, expected 0 or 1", envelope_f64);
  if (!period) return fail(MGX_E_INVALID_ARGUMENT, "period is NULL");
  if (!gauss) return fail(MGX_E_INVALID_ARGUMENT, "gauss is NULL");
  if (!penalty) return fail(MGX_E_INVALID_ARGUMENT, "penalty is NULL");
  if (!out->mask && !out->peak_offsets && !out->peaks)
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.mask, .peak_offsets and .peaks are all NULL");
  if (out->peaks && out->capacity == 0) return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.peaks is set with capacity 0");
  if (out->peak_starts && !out->starts) return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.peak_starts is set without starts");
  if (out->peak_starts && !out->peaks) return fail(MGX_E_INVALID_ARGUMENT, "mgx_peak_outputs.peak_starts is set without peaks");
  if (num_signals > 0 && !frame_offsets) return fail(MGX_E_INVALID_ARGUMENT, "frame_offsets is NULL");
  if (num_frames > 0 && !envelope) return fail(MGX_E_INVALID_ARGUMENT, "envelope is NULL");
  const uint64_t need = mgx::beats_workspace_bytes(num_frames, frame_offsets ? num_signals : 1);
  if (workspace_bytes < need || (need > 0 && !workspace))
    return fail(MGX_E_INVALID_ARGUMENT, "the workspace holds %llu bytes, the call needs %llu (mgx_beats_workspace_bytes)",
                (unsigned long long)workspace_bytes, (unsigned long long)need);
  if (need > 0 && reinterpret_cast<uintptr_t>(workspace) % 256 != 0)
    return fail(MGX_E_INVALID_ARGUMENT, "the workspace is not 256-byte aligned");
  if (num_frames == 0) {
    // no rows, no beats: the offsets alone (frame_offsets with num_signals = 0: no signal, one entry)
    if (!out->peak_offsets) return MGX_OK;
    const uint64_t S = frame_offsets ? num_signals : 1;
    const hipError_t e = hipMemsetAsync(out->peak_offsets, 0, (S + 1) * sizeof(uint64_t), (hipStream_t)stream);
    return e == hipSuccess ? MGX_OK : hip_fail(e, "hipMemsetAsync(peak_offsets)");
  }
  const hipError_t e = mgx::launch_beats(envelope, num_frames, envelope_f64 != 0, frame_offsets, num_signals, period, params->max_period,
                                         params->trim, gauss, penalty, local_score, cum_score, *out, workspace, (hipStream_t)stream);
  return e == hipSuccess ? MGX_OK : hip_fail(e, "beat kernel launch");
}

int mgx_beats_host(mgx_plan* p, const float* samples, uint64_t num_samples, const uint64_t* starts, uint64_t nframes,
                   const uint64_t* frame_offsets, uint64_t nsignals, const mgx_flux_request* flux, const mgx_tempo_params* tempo,
                   const float* window, const double* prior, const mgx_beat_params* params, const float* gauss, const double* penalty,
                   uint32_t* lag, uint64_t* peak_offsets, uint64_t* peaks, uint64_t capacity) {
  int rc = check_tempo_params(tempo);
  if (rc || (rc = check_beat_params(params))) return rc;
  if (tempo->num_lags - 1 > params->max_period)
    return fail(MGX_E_INVALID_ARGUMENT, "num_lags is %u: a lag may reach %u, above max_period %u", tempo->num_lags, tempo->num_lags - 1,
                params->max_period);
  if (nsignals == 0) return fail(MGX_E_INVALID_ARGUMENT, "num_signals is 0: beats are a clip's");
  if (!flux) return fail(MGX_E_INVALID_ARGUMENT, "flux is NULL");
  if (!window) return fail(MGX_E_INVALID_ARGUMENT, "window is NULL");
  if (!prior) return fail(MGX_E_INVALID_ARGUMENT, "prior is NULL");
  if (!gauss) return fail(MGX_E_INVALID_ARGUMENT, "gauss is NULL");
  if (!penalty) return fail(MGX_E_INVALID_ARGUMENT, "penalty is NULL");
  if (!peak_offsets) return fail(MGX_E_INVALID_ARGUMENT, "peak_offsets is NULL");
  if (!peaks && capacity > 0) return fail(MGX_E_INVALID_ARGUMENT, "peaks is NULL with capacity %llu", (unsigned long long)capacity);
  if (peaks && capacity == 0) return fail(MGX_E_INVALID_ARGUMENT, "peaks is set with capacity 0");
  mgx_summary_outputs none{};
  none.struct_size = sizeof(none);
  const BeatHost bh{params, gauss, penalty, peak_offsets, peaks, capacity};
  const TempoHost th{tempo, window, prior, nullptr, lag, &bh};
  return summarize_host_impl(p, samples, num_samples, starts, nframes, frame_offsets, nsignals, nullptr, nullptr, &none, nullptr, flux, 1,
                             nullptr, &th);
}

int mgx_wav_parse(const void* bytes, uint64_t len, mgx_wav_info* info) {
  if (!bytes || !info) return fail(MGX_E_INVALID_ARGUMENT, "NULL argument");
  if (info->struct_size != sizeof(mgx_wav_info))
    return fail(MGX_E_INVALID_ARGUMENT, "mgx_wav_info.struct_size is %u, expected %zu", info->struct_size, sizeof(mgx_wav_info));
  const unsigned char* b = static_cast<const unsigned char*>(bytes);
  if (len < 12 || memcmp(b, "RIFF", 4) != 0 || memcmp(b + 8, "WAVE", 4) != 0)
    return fail(MGX_E_INVALID_ARGUMENT, "not a RIFF/WAVE file");
  bool have_fmt = false;
  uint16_t tag = 0, channels = 0, bits = 0, align = 0;
  uint32_t rate = 0;
  uint64_t off = 12;
  while (off + 8 <= len) {
    const unsigned char* c = b + off;
    const uint64_t size = rd32(c + 4);
    if (memcmp(c, "fmt ", 4) == 0) {
      if (size < 16 || off + 8 + 16 > len) return fail(MGX_E_INVALID_ARGUMENT, "truncated fmt chunk");
      tag = rd16(c + 8);
      channels = rd16(c + 10);
      rate = rd32(c + 12);
      align = rd16(c + 20);
      bits = rd16(c + 22);
      if (tag == 0xFFFE) {  // WAVE_FORMAT_EXTENSIBLE: the subformat GUID starts with the real tag
        if (size < 40 || off + 8 + 26 > len) return fail(MGX_E_INVALID_ARGUMENT, "truncated WAVE_FORMAT_EXTENSIBLE fmt chunk");
        tag = rd16(c + 8 + 24);
      }
      have_fmt = true;
    } else if (memcmp(c, "data", 4) == 0) {
      if (!have_fmt) return fail(MGX_E_INVALID_ARGUMENT, "data chunk before fmt chunk");
      uint32_t fmt = 0xFFFFFFFFu;
      if (tag == 1 && bits == 8) fmt = MGX_PCM_U8;
      else if (tag == 1 && bits == 16) fmt = MGX_PCM_S16;
      else if (tag == 1 && bits == 24) fmt = MGX_PCM_S24;
      else if (tag == 1 && bits == 32) fmt = MGX_PCM_S32;
      else if (tag == 3 && bits == 32) fmt = MGX_PCM_F32;
      if (fmt == 0xFFFFFFFFu) return fail(MGX_E_UNSUPPORTED, "unsupported WAV encoding (format tag %u, %u bits)", tag, bits);
      if (channels == 0) return fail(MGX_E_INVALID_ARGUMENT, "WAV with 0 channels");
      if (align != channels * sample_bytes(fmt))
        return fail(MGX_E_INVALID_ARGUMENT, "block_align %u does not match %u channels x %u bytes", align, channels, sample_bytes(fmt));
      const uint64_t avail = len - (off + 8);
      const uint64_t data = std::min<uint64_t>(size, avail);
      info->pcm_format = fmt;
      info->channels = channels;
      info->sample_rate = rate;
      info->bits_per_sample = bits;
      info->block_align = align;
      info->data_offset = off + 8;
      info->data_bytes = data / align * align;
      info->sample_frames = data / align;
      return MGX_OK;
    }
    off += 8 + size + (size & 1);
  }
  return fail(MGX_E_INVALID_ARGUMENT, have_fmt ? "no data chunk" : "no fmt chunk");
}

int mgx_pcm_decode_device(const void* pcm, uint64_t sample_frames, uint32_t format, uint32_t channels,
                          uint32_t channel, float* out, void* stream) {
  if (sample_frames == 0) return MGX_OK;
  if (!pcm || !out) return fail(MGX_E_INVALID_ARGUMENT, "NULL pointer");
  if (!sample_bytes(format)) return fail(MGX_E_INVALID_ARGUMENT, "unknown PCM format %u", format);
  if (channels == 0 || channel >= channels) return fail(MGX_E_INVALID_ARGUMENT, "channel %u of %u", channel, channels);
  hipError_t e = mgx::launch_pcm_decode(pcm, sample_frames, format, channels, channel, out, (hipStream_t)stream);
  return e == hipSuccess ? MGX_OK : hip_fail(e, "PCM decode launch");
}

}  // extern "C"

namespace {

// mgx_extract_host_pcm (hop = N: floor(sample_frames / N) disjoint buffers) and mgx_extract_signal_host_pcm
int extract_host_pcm_impl(mgx_plan* p, const void* pcm, uint64_t pcm_bytes, uint64_t sample_frames, uint32_t format,
                          uint32_t channels, uint32_t channel, uint64_t hop, const mgx::Outputs* o) {
  const uint32_t bps = sample_bytes(format);
  if (!bps) return fail(MGX_E_INVALID_ARGUMENT, "unknown PCM format %u", format);
  if (channels == 0 || channel >= channels) return fail(MGX_E_INVALID_ARGUMENT, "channel %u of %u", channel, channels);
  if (int rc = check_outputs(*o)) return rc;
  const int n = p->n;
  const uint64_t nframes = sample_frames < (uint64_t)n ? 0 : (sample_frames - (uint64_t)n) / hop + 1;
  if (nframes == 0) return MGX_OK;
  if (!pcm) return fail(MGX_E_INVALID_ARGUMENT, "pcm is NULL");
  const uint64_t align = (uint64_t)bps * channels;
  if (sample_frames > pcm_bytes / align)
    return fail(MGX_E_INVALID_ARGUMENT, "%llu sample frames of %llu bytes exceed the %llu-byte PCM buffer",
                (unsigned long long)sample_frames, (unsigned long long)align, (unsigned long long)pcm_bytes);
  // (a chunk's span of samples, every channel: what one slot holds of the raw PCM)
  const uint64_t chunk_max = signal_chunk_frames(p, hop);
  const uint64_t chunk_bytes = ((std::min<uint64_t>(nframes, chunk_max) - 1) * hop + (uint64_t)n) * align;
  if (p->s_pcm_bytes < chunk_bytes) {
    if (p->s_copy) (void)hipStreamSynchronize(p->s_copy);
    for (int i = 0; i < 2; ++i) {
      if (p->s_pcm[i]) (void)hipFree(p->s_pcm[i]);
      p->s_pcm[i] = nullptr;
    }
    p->s_pcm_bytes = 0;
    hipError_t e = hipSetDevice(p->d.device);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc(reinterpret_cast<void**>(&p->s_pcm[i]), chunk_bytes);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(staging PCM)");
    p->s_pcm_bytes = chunk_bytes;
  }
  const unsigned char* src = static_cast<const unsigned char*>(pcm);
  return extract_host_chunked(p, nframes, hop, chunk_max, o, [&](uint64_t f0, uint64_t cnt, int slot, hipStream_t st) {
    const uint64_t span = (cnt - 1) * hop + (uint64_t)n;  // the chunk's samples, each copied and decoded once
    hipError_t e = hipMemcpyAsync(p->s_pcm[slot], src + f0 * hop * align, span * align, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(pcm)");
    e = mgx::launch_pcm_decode(p->s_pcm[slot], span, format, channels, channel, p->s_frames[slot], st);
    return e == hipSuccess ? MGX_OK : hip_fail(e, "PCM decode launch");
  });
}

}  // namespace

extern "C" {

int mgx_extract_host_pcm(mgx_plan* p, const void* pcm, uint64_t pcm_bytes, uint64_t sample_frames, uint32_t format,
                         uint32_t channels, uint32_t channel, const mgx_outputs* o) {
  if (!p || !o) return fail(MGX_E_INVALID_ARGUMENT, "NULL plan or outputs");
  return mgx_extract_host_pcm_ex(p, pcm, pcm_bytes, sample_frames, format, channels, channel, (uint32_t)p->n, o, nullptr);
}

int mgx_extract_signal_host_pcm(mgx_plan* p, const void* pcm, uint64_t pcm_bytes, uint64_t sample_frames, uint32_t format,
                                uint32_t channels, uint32_t channel, uint32_t hop, const mgx_outputs* o) {
  return mgx_extract_host_pcm_ex(p, pcm, pcm_bytes, sample_frames, format, channels, channel, hop, o, nullptr);
}

int mgx_extract_host_pcm_ex(mgx_plan* p, const void* pcm, uint64_t pcm_bytes, uint64_t sample_frames, uint32_t format,
                            uint32_t channels, uint32_t channel, uint32_t hop, const mgx_outputs* o,
                            const mgx_aux_outputs* aux) {
  // (a NULL plan or outputs is reported before the hop, the hop before the auxiliary struct)
  if (p && o && hop == 0) return fail(MGX_E_INVALID_ARGUMENT, "hop is 0 (a hop of at least one sample)");
  mgx::Outputs x;
  const int rc = make_outputs(p, o, aux, &x);
  if (rc) return rc;
  return extract_host_pcm_impl(p, pcm, pcm_bytes, sample_frames, format, channels, channel, hop, &x);
}

int mgx_synth_frames_device(float* frames, uint64_t nframes, uint32_t n, uint64_t seed, uint64_t first_frame, void* stream) {
  if (!frames && nframes) return fail(MGX_E_INVALID_ARGUMENT, "frames is NULL");
  if (nframes == 0) return MGX_OK;
  hipError_t e = mgx::launch_synth(frames, nframes * (uint64_t)n, seed, first_frame * (uint64_t)n, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "synth kernel launch");
  return MGX_OK;
}

}  // extern "C"
