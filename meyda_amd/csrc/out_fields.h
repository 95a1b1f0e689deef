// The table of output fields: which arrays a launch writes, the bytes of a frame in each, and how a set of them
// lies in one buffer. Host code only, no HIP: the host paths (plan.cpp), the groups (group.cpp) and
// tools/asan/host_checks.cpp include it. The N-API addon is C against the public header alone and keeps its own
// copy (meyda_amd/addon/meyda_napi.c field_bytes / set_field): an output added here is added there.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/meyda_gpu.h"

namespace mgx {

// The output arrays a launch writes: the fields of mgx_outputs, then the ones that came after its layout was
// fixed (mgx_aux_outputs of the mgx_extract_*_ex calls). The plan code and the kernels pass this around;
// the public entry points build it from the caller's two structs (plan.cpp make_outputs).
struct Outputs {
  void* scalars[MGX_NUM_SCALARS];
  float* loudness_specific;
  float* mfcc;
  float* amplitude_spectrum;
  float* power_spectrum;
  float* complex_real;
  float* complex_imag;
  float* mel_bands;  // num_frames x nfilt: the log mel energies the DCT reads (mfcc.js:53-65)
};
static_assert(offsetof(Outputs, mel_bands) == sizeof(mgx_outputs) && offsetof(Outputs, mfcc) == offsetof(mgx_outputs, mfcc) &&
                  offsetof(Outputs, complex_imag) == offsetof(mgx_outputs, complex_imag),
              "Outputs begins with mgx_outputs");
// ... so the caller's struct becomes one by copying it over the beginning, and comes back the same way
inline Outputs from_public(const mgx_outputs& o) {
  Outputs r{};
  memcpy(&r, &o, sizeof o);
  return r;
}
inline mgx_outputs public_part(const Outputs& o) {
  mgx_outputs r;
  memcpy(&r, &o, sizeof r);
  return r;
}

// Field i: 0..12 the scalars, then 13 loudness_specific .. 18 complex_imag -- the numbering of mgx_packed_layout
// and MGX_OUT_* -- and 19 mel_bands. The groups gather the first kGroupFields, the fields of mgx_outputs.
constexpr int kOutFields = 20;
constexpr int kGroupFields = 19;
constexpr int kArrayFields = kOutFields - MGX_NUM_SCALARS;
constexpr uint32_t kGroupFieldBits = (1u << kGroupFields) - 1;
// The four spectrum arrays (N/2 or N floats a frame): too long to be waited on word by word (plan.cpp wait_output_words)
constexpr uint32_t kSpectrumFieldBits = 0xFu << 15;

// Bytes per frame of field i. (The descriptor's num_bark_bands is the one definition of the loudness row:
// validate() in plan.cpp admits no other value than mgx::kBark.)
inline uint64_t out_field_bytes(const mgx_plan_desc& d, int i) {
  const uint64_t n = d.buffer_size;
  const uint64_t floats[] = {d.num_bark_bands, d.num_mfcc_coeffs, n / 2, n / 2, n, n, d.num_mel_bands};
  static_assert(sizeof floats / sizeof *floats == kArrayFields, "one entry per array field");
  return i < MGX_NUM_SCALARS ? (d.scalar_f64 ? 8 : 4) : 4 * floats[i - MGX_NUM_SCALARS];
}

// Field i's pointer
inline void*& out_field(Outputs& o, int i) {
  float** const arrays[] = {&o.loudness_specific, &o.mfcc,         &o.amplitude_spectrum, &o.power_spectrum,
                            &o.complex_real,      &o.complex_imag, &o.mel_bands};
  static_assert(sizeof arrays / sizeof *arrays == kArrayFields, "one entry per array field");
  return i < MGX_NUM_SCALARS ? o.scalars[i] : reinterpret_cast<void*&>(*arrays[i - MGX_NUM_SCALARS]);
}
inline void* out_field(const Outputs& o, int i) { return out_field(const_cast<Outputs&>(o), i); }

// Bit i: field i is requested (its pointer is not null)
inline uint32_t out_requested(const Outputs& o) {
  uint32_t bits = 0;
  for (int i = 0; i < kOutFields; ++i) bits |= out_field(o, i) ? 1u << i : 0u;
  return bits;
}

// complex_real and complex_imag come as a pair: MGX_OK, or MGX_E_INVALID_ARGUMENT and the message in *why
inline int outputs_ok(const Outputs& o, const char** why) {
  if ((o.complex_real == nullptr) == (o.complex_imag == nullptr)) return MGX_OK;
  *why = "complex_real and complex_imag must be given together";
  return MGX_E_INVALID_ARGUMENT;
}

// The fields `present` (of the first nfields) for nframes frames in one buffer, in field order, each array
// rounded up to 256 bytes: off[i] is field i's offset, UINT64_MAX for a field not present (off may be null);
// returns the buffer's bytes. mgx_packed_layout is this over the group fields.
inline uint64_t out_layout(const mgx_plan_desc& d, uint32_t present, uint64_t nframes, uint64_t* off, int nfields = kOutFields) {
  uint64_t at = 0;
  for (int i = 0; i < nfields; ++i) {
    const bool in = (present >> i) & 1u;
    if (off) off[i] = in ? at : UINT64_MAX;
    if (in) at += (out_field_bytes(d, i) * nframes + 255) / 256 * 256;
  }
  return at;
}
// What the roundings add to the arrays' own bytes, at most: one per field, and one spare
constexpr uint64_t kOutLayoutSlack = (kOutFields + 1) * 256;

// The laid-out fields as pointers into the buffer at `base`
inline Outputs out_at(unsigned char* base, const uint64_t* off, int nfields = kOutFields) {
  Outputs r{};
  for (int i = 0; i < nfields; ++i)
    if (off[i] != UINT64_MAX) out_field(r, i) = base + off[i];
  return r;
}

}  // namespace mgx
