// Host-side memory-safety run of the C ABI (built with ASan + UBSan by `make asan`; no GPU
// needed): the RIFF/WAVE walk (mgx_wav_parse) over a seeded fuzz corpus of valid files of
// every format and mutations of them (truncation at every length, byte flips, chunk sizes
// 0 / odd / huge, fmt chunks of 14-40 bytes, chunks in any order, no data), each handed over
// in a heap block of exactly its length so any over-read is caught; the host tables for
// every power-of-two buffer size up to 65536 and every mel-band / coefficient count, into
// exactly-sized buffers; shard and packed-layout arithmetic; descriptor and argument
// validation (the reference validates its inputs at src/meyda.js:20-26).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../include/meyda_gpu.h"
#include "../../meyda_amd/csrc/out_fields.h"

static int failures = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static void put16(std::vector<uint8_t>& b, uint16_t v) { b.push_back(v & 255); b.push_back(v >> 8); }
static void put32(std::vector<uint8_t>& b, uint32_t v) { for (int i = 0; i < 4; ++i) b.push_back((v >> (8 * i)) & 255); }
static void tag(std::vector<uint8_t>& b, const char* t) { b.insert(b.end(), t, t + 4); }

// A WAVE file: fmt chunk of fmt_size bytes (16, 18 or 40), optional extra chunk, data.
static std::vector<uint8_t> wav(uint16_t fmt_tag, uint16_t ch, uint16_t bits, uint32_t frames, uint32_t fmt_size,
                                bool extra_first, std::mt19937& rng) {
  std::vector<uint8_t> b;
  tag(b, "RIFF");
  put32(b, 0);
  tag(b, "WAVE");
  auto extra = [&]() {
    tag(b, "LIST");
    const uint32_t n = rng() % 7;
    put32(b, n);
    for (uint32_t i = 0; i < n; ++i) b.push_back(rng() & 255);
    if (n & 1) b.push_back(0);
  };
  if (extra_first) extra();
  tag(b, "fmt ");
  put32(b, fmt_size);
  const uint16_t align = ch * (bits / 8);
  put16(b, fmt_size == 40 ? 0xFFFE : fmt_tag);
  put16(b, ch);
  put32(b, 44100);
  put32(b, 44100u * align);
  put16(b, align);
  put16(b, bits);
  if (fmt_size >= 18) put16(b, fmt_size - 18);
  if (fmt_size == 40) {
    put16(b, bits);
    put32(b, 3);
    put16(b, fmt_tag);
    for (int i = 0; i < 14; ++i) b.push_back(0);
  }
  if (!extra_first) extra();
  tag(b, "data");
  put32(b, frames * align);
  for (uint32_t i = 0; i < frames * align; ++i) b.push_back(rng() & 255);
  const uint32_t riff = (uint32_t)b.size() - 8;
  memcpy(&b[4], &riff, 4);
  return b;
}

static void parse_exact(const std::vector<uint8_t>& bytes, size_t len) {
  uint8_t* p = static_cast<uint8_t*>(malloc(len ? len : 1));
  if (len) memcpy(p, bytes.data(), len);
  mgx_wav_info wi;
  memset(&wi, 0, sizeof wi);
  wi.struct_size = sizeof wi;
  if (mgx_wav_parse(p, len, &wi) == MGX_OK) {
    CHECK(wi.data_offset + wi.data_bytes <= len);
    CHECK(wi.block_align > 0 && wi.data_bytes % wi.block_align == 0);
    CHECK(wi.sample_frames * wi.block_align == wi.data_bytes);
    CHECK(wi.channels > 0);
  }
  free(p);
}

static void wav_fuzz() {
  std::mt19937 rng(0x6D657964);
  const struct { uint16_t t, bits; } fmts[] = {{1, 8}, {1, 16}, {1, 24}, {1, 32}, {3, 32}};
  long n = 0;
  for (const auto& f : fmts)
    for (uint16_t ch : {1, 2, 5})
      for (uint32_t fs : {16u, 18u, 40u})
        for (bool ex : {false, true}) {
          const std::vector<uint8_t> good = wav(f.t, ch, f.bits, 1 + rng() % 9, fs, ex, rng);
          mgx_wav_info wi;
          memset(&wi, 0, sizeof wi);
          wi.struct_size = sizeof wi;
          CHECK(mgx_wav_parse(good.data(), good.size(), &wi) == MGX_OK);
          for (size_t len = 0; len <= good.size(); ++len, ++n) parse_exact(good, len);  // every truncation
          for (int m = 0; m < 200; ++m, ++n) {                                       // random mutations
            std::vector<uint8_t> b = good;
            const int kind = rng() % 4;
            const size_t at = rng() % b.size();
            if (kind == 0) b[at] ^= (uint8_t)(1u << (rng() % 8));
            else if (kind == 1 && b.size() >= 4) {  // a chunk size field: 0, odd, huge, all ones
              const uint32_t vals[] = {0u, 1u, 0x7FFFFFFFu, 0xFFFFFFFFu, (uint32_t)b.size(), 13u};
              const uint32_t v = vals[rng() % 6];
              const size_t pos = std::min(at, b.size() - 4);
              memcpy(&b[pos], &v, 4);
            } else if (kind == 2) {
              b.resize(at);
            } else {
              b.insert(b.begin() + at, (size_t)(rng() % 5), (uint8_t)(rng() & 255));
            }
            parse_exact(b, b.size());
          }
        }
  // a fmt chunk shorter than 16 bytes, a data chunk first, no chunks at all
  std::vector<uint8_t> b;
  tag(b, "RIFF"); put32(b, 20); tag(b, "WAVE"); tag(b, "fmt "); put32(b, 14);
  for (int i = 0; i < 14; ++i) b.push_back(1);
  parse_exact(b, b.size());
  b.clear();
  tag(b, "RIFF"); put32(b, 12); tag(b, "WAVE"); tag(b, "data"); put32(b, 4); put32(b, 0);
  parse_exact(b, b.size());
  b.resize(12);
  parse_exact(b, b.size());
  printf("wav_parse: %ld buffers\n", n);
}

static void host_tables() {
  long n = 0;
  for (uint32_t N = 1; N <= 65536; N <<= 1)
    for (uint32_t nf : {1u, 2u, 26u, 40u, 64u})
      for (uint32_t nc : {1u, 13u, 32u}) {
        mgx_plan_desc d;
        mgx_plan_desc_init(&d);
        d.buffer_size = N;
        d.num_mel_bands = nf;
        d.num_mfcc_coeffs = nc;
        std::vector<float> win(N), han(N), ham(N), bark(N), dct((size_t)nf * nc);
        std::vector<int32_t> lim(25), bins(nf + 2);
        mgx_host_tables t = {win.data(), han.data(), ham.data(), bark.data(), lim.data(), bins.data(), dct.data()};
        CHECK(mgx_get_host_tables(&d, &t) == MGX_OK);
        CHECK(lim[24] == (int32_t)(N / 2) - 1);
        ++n;
      }
  mgx_plan_desc d;
  mgx_plan_desc_init(&d);
  d.buffer_size = 1000;
  mgx_host_tables t = {};
  CHECK(mgx_get_host_tables(&d, &t) == MGX_E_NOT_POWER_OF_TWO);
  CHECK(mgx_get_host_tables(nullptr, &t) == MGX_E_INVALID_ARGUMENT);
  printf("host tables: %ld plans\n", n);
}

static void arithmetic() {
  for (uint64_t total : {0ull, 1ull, 7ull, 262144ull, 2097155ull})
    for (uint32_t R : {1u, 3u, 8u}) {
      uint64_t next = 0;
      for (uint32_t r = 0; r < R; ++r) {
        uint64_t s, c;
        CHECK(mgx_shard_range(total, R, r, &s, &c) == MGX_OK);
        CHECK(s == next);
        next = s + c;
      }
      CHECK(next == total);
    }
  uint64_t s, c;
  CHECK(mgx_shard_range(5, 0, 0, &s, &c) != MGX_OK);
  CHECK(mgx_shard_range(5, 2, 2, &s, &c) != MGX_OK);
  mgx_plan_desc d;
  mgx_plan_desc_init(&d);
  uint64_t off[19];
  CHECK(mgx_packed_layout(&d, MGX_OUT_ALL_MASK, 1000, off) > 0);
  for (int i = 1; i < 19; ++i) CHECK(off[i] > off[i - 1] && off[i] % 256 == 0);
  CHECK(mgx_packed_layout(nullptr, 1, 1, off) == 0);
  CHECK(mgx_feature_index(nullptr) == -1);
  CHECK(mgx_feature_index("") == -1);
  CHECK(mgx_feature_name(-1) == nullptr && mgx_feature_name(MGX_NUM_FEATURES) == nullptr);
  CHECK(mgx_is_power_of_two(0.0) == 0 && mgx_is_power_of_two(1.0) == 1 && mgx_is_power_of_two(-8.0) == 0);
}

// mgx_signals_frame_starts: exactly-sized offsets, frame_offsets and starts arrays (a write past the total,
// or a read past offsets[num_signals], is the sanitizer's to see), every start inside its own signal.
static void frame_starts() {
  long n = 0;
  for (uint32_t N : {1u, 256u, 1024u})
    for (uint32_t hop : {1u, N / 4 + 1, N, N + 3})
      for (size_t ns : {(size_t)0, (size_t)1, (size_t)7}) {
        const uint64_t lens[7] = {0, N - 1, N, (uint64_t)N + hop - 1, (uint64_t)N + hop, (uint64_t)N + 5 * hop, 3ull * N + 1};
        std::vector<uint64_t> off(ns + 1, 5);
        for (size_t s = 0; s < ns; ++s) off[s + 1] = off[s] + lens[s];
        uint64_t total = ~0ull, again = 0, want = 0;
        for (size_t s = 0; s < ns; ++s) {
          uint64_t f = 0;
          CHECK(mgx_signal_frames(lens[s], N, hop, &f) == MGX_OK);
          want += f;
        }
        CHECK(mgx_signals_frame_starts(off.data(), ns, N, hop, nullptr, nullptr, 0, &total) == MGX_OK && total == want);
        std::vector<uint64_t> fo(ns + 1), st((size_t)total);
        CHECK(mgx_signals_frame_starts(off.data(), ns, N, hop, fo.data(), st.data(), total, &again) == MGX_OK && again == total);
        CHECK(fo[0] == 0 && fo[ns] == total);
        for (size_t s = 0; s < ns; ++s)
          for (uint64_t f = fo[s]; f < fo[s + 1]; ++f)
            CHECK(st[(size_t)f] == off[s] + (f - fo[s]) * hop && st[(size_t)f] + N <= off[s + 1]);
        if (total > 0) CHECK(mgx_signals_frame_starts(off.data(), ns, N, hop, fo.data(), st.data(), total - 1, &again) == MGX_E_INVALID_ARGUMENT);
        ++n;
      }
  const uint64_t down[3] = {0, 10, 9};
  uint64_t total = 0;
  CHECK(mgx_signals_frame_starts(down, 2, 4, 1, nullptr, nullptr, 0, &total) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_signals_frame_starts(down, 1, 4, 0, nullptr, nullptr, 0, &total) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_signals_frame_starts(down, 1, 4, 1, nullptr, nullptr, 0, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_signals_frame_starts(nullptr, 1, 4, 1, nullptr, nullptr, 0, &total) == MGX_E_INVALID_ARGUMENT);
  const uint64_t one = 0;
  CHECK(mgx_extract_gather_host(nullptr, nullptr, 0, &one, 1, nullptr, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_extract_gather_device(nullptr, nullptr, 0, &one, 1, nullptr, nullptr, nullptr) == MGX_E_INVALID_ARGUMENT);
  // the summary calls: the struct is checked ahead of the plan, then the plan (nothing is read through either)
  const uint64_t fo[2] = {0, 1};
  uint64_t bytes = 77;
  mgx_summary_outputs so;
  memset(&so, 0, sizeof so);
  for (uint32_t size : {0u, (uint32_t)sizeof so - 8, (uint32_t)sizeof so + 8, (uint32_t)sizeof so}) {
    so.struct_size = size;
    CHECK(mgx_summarize_host(nullptr, nullptr, 0, &one, 1, fo, 1, nullptr, nullptr, &so) == MGX_E_INVALID_ARGUMENT);
    CHECK(strstr(mgx_last_error(), size == sizeof so ? "NULL plan" : "struct_size") != nullptr);
    CHECK(mgx_summarize_device(nullptr, nullptr, 0, &one, 1, fo, 1, nullptr, nullptr, &so, nullptr, 0, nullptr) == MGX_E_INVALID_ARGUMENT);
    CHECK(mgx_summary_workspace_bytes(nullptr, nullptr, nullptr, &so, 1, 1, &bytes) == MGX_E_INVALID_ARGUMENT);
  }
  CHECK(mgx_summarize_host(nullptr, nullptr, 0, &one, 1, fo, 1, nullptr, nullptr, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_summary_workspace_bytes(nullptr, nullptr, nullptr, &so, 1, 1, nullptr) == MGX_E_INVALID_ARGUMENT && bytes == 77);
  // the delta calls: the delta struct and the summaries it names are checked ahead of the plan too; the operator
  // refuses its arguments before any launch (no pointer is read)
  so.struct_size = sizeof so;
  mgx_summary_outputs named = so;
  double stats[4 * 13];
  named.mfcc = stats;
  mgx_delta_summaries ds{(uint32_t)sizeof(mgx_delta_summaries), 2, &named, &named};
  auto delta_calls = [&](int want, const char* why) {
    CHECK(mgx_summarize_deltas_host(nullptr, nullptr, 0, &one, 1, fo, 1, nullptr, nullptr, &so, &ds) == want);
    CHECK(strstr(mgx_last_error(), why) != nullptr);
    CHECK(mgx_summarize_deltas_device(nullptr, nullptr, 0, &one, 1, fo, 1, nullptr, nullptr, &so, &ds, nullptr, 0, nullptr) == want);
    CHECK(mgx_summarize_deltas_workspace_bytes(nullptr, nullptr, nullptr, &so, &ds, 1, 1, &bytes) == want && bytes == 77);
  };
  delta_calls(MGX_E_INVALID_ARGUMENT, "NULL plan");
  ds.width = MGX_DELTA_MAX_WIDTH + 1;
  delta_calls(MGX_E_INVALID_ARGUMENT, "width");
  ds.width = 2;
  ds.struct_size -= 8;
  delta_calls(MGX_E_INVALID_ARGUMENT, "mgx_delta_summaries.struct_size");
  ds.struct_size += 8;
  named.power_spectrum = stats;
  delta_calls(MGX_E_UNSUPPORTED, "spectrum");
  named.power_spectrum = nullptr;
  named.reserved = 1;
  delta_calls(MGX_E_INVALID_ARGUMENT, "reserved");
  float rows[4], d1[4], d2[4];
  CHECK(mgx_delta_device(rows, 4, 0, 0, nullptr, 0, 2, d1, d2, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_delta_device(rows, 4, 1, 0, nullptr, 0, 0, d1, d2, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_delta_device(rows, 4, 1, 0, nullptr, 0, 9, d1, d2, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_delta_device(rows, 4, 1, 2, nullptr, 0, 2, d1, d2, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_delta_device(rows, 4, 1, 0, nullptr, 0, 2, nullptr, nullptr, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_delta_device(rows, 4, 1, 0, nullptr, 0, 2, d1, d1, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_delta_device(rows, 4, 1, 0, nullptr, 0, 2, rows, d2, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_delta_device(rows, 4, 1, 0, nullptr, 1, 2, d1, d2, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_delta_device(nullptr, 4, 1, 0, nullptr, 0, 2, d1, d2, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_delta_device(nullptr, 0, 1, 0, nullptr, 0, 2, d1, d2, nullptr) == MGX_OK);
  printf("frame starts: %ld tables\n", n);
}

// The table of output fields (meyda_amd/csrc/out_fields.h, included as the library includes it): its accessor
// against the structs' members by name, its layout against the public mgx_packed_layout (itself pinned by
// tests/test_group_host.py against independent arithmetic), its field sets.
static void out_fields() {
  using namespace mgx;
  // field access: exactly one pointer member per field, where the public struct has it
  mgx_outputs named[kGroupFields];
  memset(named, 0, sizeof named);
  void* const mark = &named;
  for (int i = 0; i < MGX_NUM_SCALARS; ++i) named[i].scalars[i] = mark;
  named[13].loudness_specific = static_cast<float*>(mark);
  named[14].mfcc = static_cast<float*>(mark);
  named[15].amplitude_spectrum = static_cast<float*>(mark);
  named[16].power_spectrum = static_cast<float*>(mark);
  named[17].complex_real = static_cast<float*>(mark);
  named[18].complex_imag = static_cast<float*>(mark);
  for (int i = 0; i < kOutFields; ++i) {
    Outputs o;
    memset(&o, 0, sizeof o);
    out_field(o, i) = mark;
    void* members[sizeof(Outputs) / sizeof(void*)];
    static_assert(sizeof members == sizeof o, "Outputs holds pointers only");
    memcpy(members, &o, sizeof o);
    int set = 0;
    for (void* m : members) set += m != nullptr;
    CHECK(set == 1);
    CHECK(out_field(static_cast<const Outputs&>(o), i) == mark);
    if (i < kGroupFields) CHECK(memcmp(&o, &named[i], sizeof(mgx_outputs)) == 0);
    else CHECK(o.mel_bands == mark && i == 19);
    // field sets: the requested bits round-trip through the accessor
    CHECK(out_requested(o) == 1u << i);
    const char* why = nullptr;
    CHECK((outputs_ok(o, &why) == MGX_OK) == (i != 17 && i != 18));
  }
  Outputs pair{}, none{}, mel{};
  pair.complex_real = pair.complex_imag = mel.mel_bands = static_cast<float*>(mark);
  const char* why = nullptr;
  CHECK(outputs_ok(pair, &why) == MGX_OK && outputs_ok(none, &why) == MGX_OK && why == nullptr);
  pair.complex_imag = nullptr;
  CHECK(outputs_ok(pair, &why) == MGX_E_INVALID_ARGUMENT && why && strstr(why, "given together"));
  CHECK(out_requested(none) == 0 && (out_requested(mel) & kGroupFieldBits) == 0);  // mel_bands alone: resident key 0
  // layout against the public call
  std::mt19937 rng(0x6F757466);
  long n = 0;
  for (uint32_t N : {256u, 512u, 1024u, 2048u})
    for (uint32_t f64 : {0u, 1u})
      for (const auto& mc : {std::pair<uint32_t, uint32_t>{1, 1}, {26, 13}, {40, 20}, {64, 32}})
        for (uint64_t F : {1ull, 7ull, 513ull, 65536ull}) {
          mgx_plan_desc d;
          mgx_plan_desc_init(&d);
          d.buffer_size = N;
          d.scalar_f64 = f64;
          d.num_mel_bands = mc.first;
          d.num_mfcc_coeffs = mc.second;
          std::vector<uint32_t> masks;
          for (int b = 0; b < 18; ++b) masks.push_back(1u << b);
          masks.push_back(MGX_OUT_ALL_MASK);
          for (int r = 0; r < 64; ++r) masks.push_back(rng() & MGX_OUT_ALL_MASK);
          for (uint32_t mask : masks) {
            const uint32_t bits = mask | ((mask >> 17) & 1u) << 18;  // (MGX_OUT_COMPLEX_SPECTRUM: fields 17 and 18)
            uint64_t want[kGroupFields], got[kOutFields], with[kOutFields];
            const uint64_t total = mgx_packed_layout(&d, mask, F, want);
            CHECK(out_layout(d, bits, F, got, kGroupFields) == total);
            CHECK(memcmp(want, got, sizeof want) == 0);
            // with field 19: last, 256-byte aligned, its own rounded bytes more
            const uint64_t all = out_layout(d, bits | 1u << 19, F, with);
            CHECK(memcmp(want, with, sizeof want) == 0);
            CHECK(with[19] == total && with[19] % 256 == 0);
            CHECK(all == total + (4ull * mc.first * F + 255) / 256 * 256);
            CHECK(out_layout(d, bits, F, with) == total && with[19] == UINT64_MAX);
            // the pointers built from it
            unsigned char* const base = reinterpret_cast<unsigned char*>(uintptr_t(1) << 40);
            const Outputs at = out_at(base, got, kGroupFields);
            for (int i = 0; i < kOutFields; ++i)
              CHECK(out_field(at, i) == (i < kGroupFields && got[i] != UINT64_MAX ? base + got[i] : nullptr));
            ++n;
          }
        }
  static_assert(kOutLayoutSlack == 21 * 256, "one rounding per field, and a spare");
  printf("out fields: %ld layouts\n", n);
}

static void validation() {
  mgx_plan* p = nullptr;
  CHECK(mgx_plan_create(nullptr, &p) == MGX_E_INVALID_ARGUMENT);
  mgx_plan_desc d;
  mgx_plan_desc_init(&d);
  d.struct_size = 4;
  CHECK(mgx_plan_create(&d, &p) == MGX_E_INVALID_ARGUMENT);
  mgx_plan_desc_init(&d);
  d.flags = 0x80;
  CHECK(mgx_plan_create(&d, &p) == MGX_E_INVALID_ARGUMENT);
  mgx_plan_desc_init(&d);
  d.num_mel_bands = 65;
  CHECK(mgx_plan_create(&d, &p) == MGX_E_UNSUPPORTED);
  mgx_group* g = nullptr;
  CHECK(mgx_group_create(&d, nullptr, 0, &g) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_group_create_rank(&d, nullptr, 2, 5, &g) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_extract_host_pcm(nullptr, nullptr, 0, 0, 0, 0, 0, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(strlen(mgx_last_error()) > 0);
}

// mgx_beat_tables into blocks of exactly the stated sizes, for the smallest and the largest period and some between
static void beat_tables() {
  long n = 0;
  for (uint32_t P : {1u, 2u, 3u, 7u, 128u, 1022u, (uint32_t)MGX_BEAT_MAX_PERIOD}) {
    std::vector<float> gauss(((size_t)P + 1) * (P + 2) / 2, -1.0f);
    std::vector<double> penalty(((size_t)P + 1) * (P + 1), 1.0);
    CHECK(mgx_beat_tables(P, 100.0, gauss.data(), penalty.data()) == MGX_OK);
    for (float v : gauss) CHECK(v >= 0.0f && v <= 1.0f);
    for (double v : penalty) CHECK(v <= 0.0);
    CHECK(gauss[0] == 1.0f && gauss.back() == 0.0f && penalty[(size_t)P * P + P] == 0.0);
    n += (long)(gauss.size() + penalty.size());
  }
  float g1[3];
  double p1[4];
  CHECK(mgx_beat_tables(0, 100.0, g1, p1) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_beat_tables(MGX_BEAT_MAX_PERIOD + 1, 100.0, g1, p1) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_beat_tables(1, 0.0, g1, p1) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_beat_tables(1, 100.0, nullptr, p1) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_beat_tables(1, 100.0, g1, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_beat_tables(1, 100.0, g1, p1) == MGX_OK);
  uint64_t bytes = 1;
  CHECK(mgx_beats_workspace_bytes(0, 0, &bytes) == MGX_OK && bytes == 0);
  CHECK(mgx_beats_workspace_bytes(1000, 3, &bytes) == MGX_OK && bytes % 256 == 0 && bytes > 20000);
  printf("beat tables: %ld entries\n", n);
}

// mgx_hpss_params_init, and every refusal of mgx_hpss_device and mgx_hpss_host that comes before a device is touched
static void hpss_refusals() {
  mgx_hpss_params hp;
  memset(&hp, 0xFF, sizeof hp);
  mgx_hpss_params_init(&hp);
  CHECK(hp.struct_size == sizeof hp && hp.kernel_time == 31 && hp.kernel_freq == 31 && hp.mode == MGX_HPSS_SOFT2);
  CHECK(hp.margin_harmonic == 1.0f && hp.margin_percussive == 1.0f);
  mgx_hpss_params_init(nullptr);
  uint32_t tr = 0, tc = 0;
  mgx_hpss_tile(&tr, &tc);
  mgx_hpss_tile(nullptr, nullptr);
  CHECK(tr == MGX_HPSS_TILE_ROWS && tc == MGX_HPSS_TILE_COLS);
  float block[12];
  float *rows = block, *h = block + 4, *p = block + 8;  // (never read: every call below is refused or has no rows)
  auto dev = [&](const mgx_hpss_params* q) { return mgx_hpss_device(rows, 4, 1, nullptr, 0, q, h, p, nullptr); };
  auto host = [&](const mgx_hpss_params* q) {
    return mgx_hpss_host(nullptr, nullptr, 0, nullptr, 0, nullptr, 1, q, nullptr, nullptr, h, nullptr);
  };
  long n = 0;
  auto both = [&](mgx_hpss_params q, const char* why) {
    CHECK(dev(&q) == MGX_E_INVALID_ARGUMENT && strstr(mgx_last_error(), why) != nullptr);
    CHECK(host(&q) == MGX_E_INVALID_ARGUMENT && strstr(mgx_last_error(), why) != nullptr);
    ++n;
  };
  mgx_hpss_params q = hp;
  q.struct_size = 20; both(q, "struct_size"); q = hp;
  for (uint32_t k : {0u, 2u, 30u, 33u, 0x80000001u}) {
    q.kernel_time = k; both(q, "kernel_time"); q = hp;
    q.kernel_freq = k; both(q, "kernel_freq"); q = hp;
  }
  for (uint32_t m : {4u, 0x80000000u}) { q.mode = m; both(q, "mode"); q = hp; }
  for (float m : {0.5f, -1.0f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()}) {
    q.margin_harmonic = m; both(q, "margin_harmonic"); q = hp;
    q.margin_percussive = m; both(q, "margin_percussive"); q = hp;
  }
  CHECK(dev(nullptr) == MGX_E_INVALID_ARGUMENT && host(nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_hpss_device(rows, 4, 0, nullptr, 0, &hp, h, p, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_hpss_device(rows, 4, 1, nullptr, 0, &hp, nullptr, nullptr, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_hpss_device(rows, 4, 1, nullptr, 0, &hp, h, h, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_hpss_device(rows, 4, 1, nullptr, 0, &hp, rows, p, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_hpss_device(rows, 4, 1, nullptr, 0, &hp, h, rows, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_hpss_device(rows, 4, 1, nullptr, 1, &hp, h, p, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_hpss_device(nullptr, 4, 1, nullptr, 0, &hp, h, p, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(mgx_hpss_device(nullptr, 0, 1, nullptr, 0, &hp, h, nullptr, nullptr) == MGX_OK);
  // the host call: its own refusals and the requests', all ahead of the plan
  CHECK(mgx_hpss_host(nullptr, nullptr, 0, nullptr, 0, nullptr, 1, &hp, nullptr, nullptr, nullptr, nullptr) == MGX_E_INVALID_ARGUMENT);
  CHECK(strstr(mgx_last_error(), "all NULL") != nullptr);
  CHECK(mgx_hpss_host(nullptr, nullptr, 0, nullptr, 0, nullptr, 1, &hp, nullptr, nullptr, h, h) == MGX_E_INVALID_ARGUMENT);
  float w[2] = {1.0f, 1.0f}, pf[2];
  double sm[8];
  mgx_chroma_request cr{};
  cr.struct_size = sizeof cr;
  cr.num_chroma = 1;
  cr.norm = MGX_CHROMA_NORM_MAX;
  cr.weights = w;
  cr.per_frame = pf;
  auto with_chroma = [&](mgx_chroma_request c, uint64_t S) {
    return mgx_hpss_host(nullptr, nullptr, 0, nullptr, 0, nullptr, S, &hp, &c, nullptr, nullptr, nullptr);
  };
  mgx_chroma_request c = cr;
  c.struct_size = 32; CHECK(with_chroma(c, 1) == MGX_E_INVALID_ARGUMENT); c = cr;
  c.num_chroma = MGX_CHROMA_MAX_BINS + 1; CHECK(with_chroma(c, 1) == MGX_E_INVALID_ARGUMENT); c = cr;
  c.norm = MGX_NUM_CHROMA_NORMS; CHECK(with_chroma(c, 1) == MGX_E_INVALID_ARGUMENT); c = cr;
  c.weights = nullptr; CHECK(with_chroma(c, 1) == MGX_E_INVALID_ARGUMENT); c = cr;
  c.per_frame = nullptr; CHECK(with_chroma(c, 1) == MGX_E_INVALID_ARGUMENT); c = cr;
  c.summary = sm; CHECK(with_chroma(c, 0) == MGX_E_INVALID_ARGUMENT); c = cr;
  CHECK(with_chroma(cr, 1) == MGX_E_INVALID_ARGUMENT && strstr(mgx_last_error(), "plan is NULL") != nullptr);
  mgx_flux_request fr{};
  fr.struct_size = sizeof fr;
  fr.field = MGX_AMPLITUDE_SPECTRUM;
  fr.mode = MGX_FLUX_RECTIFIED;
  fr.lag = 1;
  fr.per_frame = pf;
  auto with_flux = [&](mgx_flux_request f, uint64_t S) {
    return mgx_hpss_host(nullptr, nullptr, 0, nullptr, 0, nullptr, S, &hp, nullptr, &f, nullptr, nullptr);
  };
  mgx_flux_request f = fr;
  f.struct_size = 24; CHECK(with_flux(f, 1) == MGX_E_INVALID_ARGUMENT); f = fr;
  f.mode = MGX_NUM_FLUX_MODES; CHECK(with_flux(f, 1) == MGX_E_INVALID_ARGUMENT); f = fr;
  f.lag = 0; CHECK(with_flux(f, 1) == MGX_E_INVALID_ARGUMENT); f = fr;
  f.lag = MGX_FLUX_MAX_LAG + 1; CHECK(with_flux(f, 1) == MGX_E_INVALID_ARGUMENT); f = fr;
  f.per_frame = nullptr; CHECK(with_flux(f, 1) == MGX_E_INVALID_ARGUMENT); f = fr;
  f.summary = sm; CHECK(with_flux(f, 0) == MGX_E_INVALID_ARGUMENT); f = fr;
  f.field = MGX_MFCC; CHECK(with_flux(f, 1) == MGX_E_UNSUPPORTED); f = fr;
  f.field = MGX_RMS; CHECK(with_flux(f, 1) == MGX_E_UNSUPPORTED); f = fr;
  CHECK(with_flux(fr, 1) == MGX_E_INVALID_ARGUMENT && strstr(mgx_last_error(), "plan is NULL") != nullptr);
  printf("hpss refusals: %ld parameter sets through both calls\n", n);
}

int main() {
  wav_fuzz();
  host_tables();
  beat_tables();
  hpss_refusals();
  arithmetic();
  frame_starts();
  out_fields();
  validation();
  printf("host_checks: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
