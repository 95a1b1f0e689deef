"""ctypes binding of the C ABI in include/meyda_gpu.h (libmeyda_gpu.so, built in-tree).

This is plumbing for the Python test suite and bench.py; the product host binding
for the reference's JavaScript API is the N-API addon (meyda_amd/addon/) used by
meyda_amd/js/meyda.js. There is no CPU fallback here: if the HIP library is
missing or no gfx950 device is present, every compute call raises.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MEYDA_AMD_LIB") or os.path.join(HERE, "libmeyda_gpu.so")

NUM_SCALARS = 13
NUM_BARK = 24
SCALAR_NAMES = ["rms", "energy", "zcr", "spectralCentroid", "spectralFlatness", "spectralSlope",
                "spectralRolloff", "spectralSpread", "spectralSkewness", "spectralKurtosis",
                "loudness.total", "perceptualSpread", "perceptualSharpness"]
FEATURE_NAMES = SCALAR_NAMES + ["loudness", "mfcc", "amplitudeSpectrum", "powerSpectrum",
                                "complexSpectrum", "buffer", "melBands"]
WINDOWS = {"hanning": 0, "hamming": 1}
PRECISIONS = {"faithful": 0, "fast": 1}
MODES = {"per_buffer_fft": 0, "literal": 1}

STATUS = {0: "MGX_OK", -1: "MGX_E_INVALID_ARGUMENT", -2: "MGX_E_NOT_POWER_OF_TWO",
          -3: "MGX_E_UNSUPPORTED", -4: "MGX_E_DEVICE", -5: "MGX_E_OUT_OF_MEMORY",
          -6: "MGX_E_NO_DEVICE"}

# Every symbol include/meyda_gpu.h declares (checked by tests/test_capi_host.py).
EXPORTS = ["mgx_plan_desc_init", "mgx_plan_create", "mgx_plan_destroy", "mgx_plan_get_desc",
           "mgx_extract_device", "mgx_extract_host", "mgx_synth_frames_device",
           "mgx_get_host_tables", "mgx_is_power_of_two", "mgx_feature_index", "mgx_feature_name",
           "mgx_feature_info", "mgx_device_count", "mgx_abi_version", "mgx_last_error",
           "mgx_wav_parse", "mgx_pcm_decode_device", "mgx_extract_host_pcm",
           "mgx_signal_frames", "mgx_extract_signal_device", "mgx_extract_signal_host",
           "mgx_extract_signal_host_pcm",
           "mgx_extract_device_ex", "mgx_extract_host_ex", "mgx_extract_host_pcm_ex",
           "mgx_signals_frame_starts", "mgx_extract_gather_device", "mgx_extract_gather_host",
           "mgx_summary_workspace_bytes", "mgx_summarize_device", "mgx_summarize_host",
           "mgx_delta_device", "mgx_summarize_deltas_workspace_bytes", "mgx_summarize_deltas_device",
           "mgx_summarize_deltas_host",
           "mgx_flux_device", "mgx_summarize_flux_workspace_bytes", "mgx_summarize_flux_device", "mgx_summarize_flux_host",
           "mgx_peaks_workspace_bytes", "mgx_peaks_device", "mgx_onsets_host",
           "mgx_chroma_params_init", "mgx_chroma_weights", "mgx_chroma_device", "mgx_chroma_host",
           "mgx_tempo_params_init", "mgx_tempogram_window", "mgx_tempo_prior", "mgx_tempogram_device",
           "mgx_tempo_workspace_bytes", "mgx_tempo_device", "mgx_tempo_host",
           "mgx_beat_params_init", "mgx_beat_tables", "mgx_beats_workspace_bytes", "mgx_beats_device", "mgx_beats_host",
           "mgx_hpss_params_init", "mgx_hpss_tile", "mgx_hpss_device", "mgx_hpss_host",
           "mgx_shard_range", "mgx_packed_layout", "mgx_comm_unique_id", "mgx_group_create",
           "mgx_group_create_rank", "mgx_group_create_loopback", "mgx_group_create_loopback_rccl", "mgx_group_destroy",
           "mgx_group_info", "mgx_group_comm_info", "mgx_group_extract_device", "mgx_group_extract_host"]
COMM_ID_BYTES = 128
FLAG_DCT_SEQUENTIAL = 1  # mgx_plan_desc.flags
FLAG_MFCC_REFERENCE = 2  # mel sums, log and DCT in the reference's own order
FLAG_RESIDENT = 4  # one-frame host calls served by a workgroup that stays on the device (include/meyda_gpu.h)
# output selection bits of a group extraction (MGX_OUT_* in include/meyda_gpu.h)
OUT_LOUDNESS_SPECIFIC, OUT_MFCC, OUT_AMPLITUDE, OUT_POWER, OUT_COMPLEX = (1 << 13, 1 << 14, 1 << 15, 1 << 16,
                                                                          1 << 17)
# field order of mgx_packed_layout / mgx_outputs
FIELDS = SCALAR_NAMES + ["loudness.specific", "mfcc", "amplitudeSpectrum", "powerSpectrum",
                         "complexSpectrum.real", "complexSpectrum.imag"]
PCM_FORMATS = {"f32": 0, "s16": 1, "u8": 2, "s24": 3, "s32": 4}


class MgxError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s (%d): %s" % (STATUS.get(status, "?"), status, message))
        self.status = status


class PlanDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("buffer_size", ctypes.c_uint32),
                ("sample_rate", ctypes.c_double), ("window", ctypes.c_uint32),
                ("precision", ctypes.c_uint32), ("mode", ctypes.c_uint32),
                ("num_bark_bands", ctypes.c_uint32), ("num_mel_bands", ctypes.c_uint32),
                ("num_mfcc_coeffs", ctypes.c_uint32), ("scalar_f64", ctypes.c_uint32),
                ("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class Outputs(ctypes.Structure):
    _fields_ = [("scalars", ctypes.c_void_p * NUM_SCALARS),
                ("loudness_specific", ctypes.c_void_p), ("mfcc", ctypes.c_void_p),
                ("amplitude_spectrum", ctypes.c_void_p), ("power_spectrum", ctypes.c_void_p),
                ("complex_real", ctypes.c_void_p), ("complex_imag", ctypes.c_void_p)]


class AuxOutputs(ctypes.Structure):
    """mgx_aux_outputs: the outputs added after mgx_outputs (the mgx_extract_*_ex calls)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("mel_bands", ctypes.c_void_p)]


def _aux(outputs):
    """The AuxOutputs that alloc_outputs / _host_outputs hung on `outputs` ("melBands" requested), or None."""
    return getattr(outputs, "aux", None)


def _aux_ref(outputs):
    a = _aux(outputs)
    return None if a is None else ctypes.byref(a)


def _set_mel_bands(outputs, ptr):
    a = AuxOutputs()
    a.struct_size = ctypes.sizeof(AuxOutputs)
    a.mel_bands = ptr
    outputs.aux = a  # (a Python attribute of the Outputs instance: the C struct is unchanged)


STATS = ["mean", "variance", "min", "max"]  # mgx_stat
# the fields a summary pools (mgx_summary_outputs), by feature name; "loudness" stands for specific and total
SUMMARY_FEATURES = SCALAR_NAMES + ["loudness", "mfcc", "amplitudeSpectrum", "powerSpectrum", "melBands"]


class SummaryOutputs(ctypes.Structure):
    """mgx_summary_outputs: per pooled field, num_signals x 4 x width float64 (the mgx_summarize_* calls)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("scalars", ctypes.c_void_p * NUM_SCALARS),
                ("loudness_specific", ctypes.c_void_p), ("mfcc", ctypes.c_void_p),
                ("amplitude_spectrum", ctypes.c_void_p), ("power_spectrum", ctypes.c_void_p),
                ("mel_bands", ctypes.c_void_p)]


DELTA_MAX_WIDTH = 8  # MGX_DELTA_MAX_WIDTH
# the fields whose delta rows a summary call pools (mgx_delta_summaries): SUMMARY_FEATURES less the spectra
DELTA_FEATURES = SCALAR_NAMES + ["loudness", "mfcc", "melBands"]


class DeltaSummaries(ctypes.Structure):
    """mgx_delta_summaries: the summaries of the delta and second-order rows (the mgx_summarize_deltas_* calls)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("delta", ctypes.POINTER(SummaryOutputs)), ("delta2", ctypes.POINTER(SummaryOutputs))]


FLUX_MODES = {"rectified": 0, "l1": 1, "l2": 2}  # mgx_flux_mode
FLUX_MAX_LAG = 8  # MGX_FLUX_MAX_LAG
FLUX_MAX_REQUESTS = 4  # MGX_FLUX_MAX_REQUESTS
# the fields a summary call takes the flux of (mgx_flux_request.field), by feature name; "loudness": its specific rows
FLUX_FEATURES = {"loudness": 13, "mfcc": 14, "amplitudeSpectrum": 15, "powerSpectrum": 16, "melBands": 19}


class FluxRequest(ctypes.Structure):
    """mgx_flux_request: one flux of one field through the mgx_summarize_flux_* calls."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("field", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("lag", ctypes.c_uint32),
                ("per_frame", ctypes.c_void_p), ("summary", ctypes.c_void_p)]


PEAK_MAX_REACH = 64  # MGX_PEAK_MAX_REACH
PEAK_PARAMS = ("pre_max", "post_max", "pre_avg", "post_avg", "delta", "wait")


class PeakParams(ctypes.Structure):
    """mgx_peak_params: the windows, the threshold and the minimum distance of the peak picker."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("pre_max", ctypes.c_uint32), ("post_max", ctypes.c_uint32),
                ("pre_avg", ctypes.c_uint32), ("post_avg", ctypes.c_uint32), ("wait", ctypes.c_uint32),
                ("delta", ctypes.c_double)]


class PeakOutputs(ctypes.Structure):
    """mgx_peak_outputs: what mgx_peaks_device writes (device pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("mask", ctypes.c_void_p),
                ("peak_offsets", ctypes.c_void_p), ("peaks", ctypes.c_void_p), ("capacity", ctypes.c_uint64),
                ("starts", ctypes.c_void_p), ("peak_starts", ctypes.c_void_p)]


def peak_params(pre_max=0, post_max=0, pre_avg=0, post_avg=0, delta=0.0, wait=0):
    """A PeakParams; numbers out of range pass through: the library refuses them with its message."""
    p = PeakParams()
    p.struct_size = ctypes.sizeof(PeakParams)
    p.pre_max, p.post_max, p.pre_avg, p.post_avg, p.wait, p.delta = pre_max, post_max, pre_avg, post_avg, wait, delta
    return p


CHROMA_MAX_BINS = 36  # MGX_CHROMA_MAX_BINS
CHROMA_NORMS = {"none": 0, "max": 1}  # mgx_chroma_norm
CHROMA_PARAMS = ("num_chroma", "a440", "center_octave", "octave_width", "base_c")


class ChromaParams(ctypes.Structure):
    """mgx_chroma_params: the construction of the chroma filter bank (mgx_chroma_weights)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_chroma", ctypes.c_uint32), ("a440", ctypes.c_double),
                ("center_octave", ctypes.c_double), ("octave_width", ctypes.c_double), ("base_c", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class ChromaRequest(ctypes.Structure):
    """mgx_chroma_request: what mgx_chroma_host computes and where it goes (host pointers)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("num_chroma", ctypes.c_uint32), ("norm", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("weights", ctypes.c_void_p), ("per_frame", ctypes.c_void_p),
                ("summary", ctypes.c_void_p)]


TEMPOGRAM_MAX_WIN = 1024  # MGX_TEMPOGRAM_MAX_WIN
TEMPO_CHUNK_ROWS = 65536  # MGX_TEMPO_CHUNK_ROWS
TEMPOGRAM_NORMS = {"none": 0, "lag0": 1}  # mgx_tempogram_norm
TEMPO_PARAMS = ("win_length", "num_lags", "norm", "gain")


class TempoParams(ctypes.Structure):
    """mgx_tempo_params: the window length, the lags, the normalisation of the tempogram and the gain of the pick."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("win_length", ctypes.c_uint32), ("num_lags", ctypes.c_uint32),
                ("norm", ctypes.c_uint32), ("gain", ctypes.c_double)]


BEAT_MAX_PERIOD = 1023  # MGX_BEAT_MAX_PERIOD


class BeatParams(ctypes.Structure):
    """mgx_beat_params: the size of the tables and the trim of the beat tracker."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_period", ctypes.c_uint32), ("trim", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def beat_params(max_period=None, trim=None):
    """A BeatParams with the library's defaults (mgx_beat_params_init: 1023, trim) and the arguments over them.
    Numbers out of range pass through: the library refuses them."""
    p = BeatParams()
    lib().mgx_beat_params_init(ctypes.byref(p))
    if max_period is not None:
        p.max_period = int(max_period)
    if trim is not None:
        p.trim = int(trim)
    return p


def _tempogram_norm(norm):
    if isinstance(norm, str):
        if norm not in TEMPOGRAM_NORMS:
            raise ValueError("tempogram norm %r: one of %s" % (norm, sorted(TEMPOGRAM_NORMS)))
        return TEMPOGRAM_NORMS[norm]
    return int(norm)


def tempo_params(win_length=None, num_lags=None, norm=None, gain=None):
    """A TempoParams with the library's defaults (mgx_tempo_params_init: 384, 384, "lag0", 1e6) and the arguments
    over them; num_lags defaults to win_length. Numbers out of range pass through: the library refuses them."""
    p = TempoParams()
    lib().mgx_tempo_params_init(ctypes.byref(p))
    if win_length is not None:
        p.win_length = p.num_lags = int(win_length)
    if num_lags is not None:
        p.num_lags = int(num_lags)
    if norm is not None:
        p.norm = _tempogram_norm(norm)
    if gain is not None:
        p.gain = float(gain)
    return p


HPSS_MODES = {"medians": 0, "soft1": 1, "soft2": 2, "hard": 3}  # mgx_hpss_mode
HPSS_MAX_KERNEL = 31


class HpssParams(ctypes.Structure):
    """mgx_hpss_params: the two median kernels, the mode and the margins of mgx_hpss_device / mgx_hpss_host."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("kernel_time", ctypes.c_uint32), ("kernel_freq", ctypes.c_uint32),
                ("mode", ctypes.c_uint32), ("margin_harmonic", ctypes.c_float), ("margin_percussive", ctypes.c_float)]


def _pair(v, what):
    """A value for both sides, or one for each: (time, frequency) or (harmonic, percussive)."""
    if isinstance(v, (tuple, list, np.ndarray)):
        if len(v) != 2:
            raise TypeError("%s: one value or a pair" % what)
        return v[0], v[1]
    return v, v


def hpss_params(kernel_size=None, mode=None, margin=None, power=None):
    """An HpssParams with the library's defaults (mgx_hpss_params_init: kernels 31 x 31, "soft2", margins 1) and the
    arguments over them. kernel_size: one odd size or (time, frequency); margin: one value or (harmonic, percussive);
    mode: "medians", "soft1", "soft2", "hard" or the enum's number; power: librosa's name for the mode (1, 2 or
    inf) instead of it. Numbers out of range are refused by the library, not here."""
    p = HpssParams()
    lib().mgx_hpss_params_init(ctypes.byref(p))
    if kernel_size is not None:
        kt, kf = _pair(kernel_size, "kernel_size")
        p.kernel_time, p.kernel_freq = int(kt), int(kf)
    if power is not None:
        if mode is not None:
            raise TypeError("hpss: mode or power, not both")
        if power not in (1, 2, float("inf")):
            raise ValueError("hpss power %r: 1, 2 or inf" % (power,))
        mode = "hard" if power == float("inf") else "soft%d" % int(power)
    if mode is not None:
        if isinstance(mode, str):
            if mode not in HPSS_MODES:
                raise ValueError("hpss mode %r: one of %s" % (mode, sorted(HPSS_MODES)))
            mode = HPSS_MODES[mode]
        p.mode = int(mode)
    if margin is not None:
        mh, mp = _pair(margin, "margin")
        p.margin_harmonic, p.margin_percussive = float(mh), float(mp)
    return p


def hpss_tile():
    """(rows, columns) of the tile a workgroup of the HPSS kernel owns (mgx_hpss_tile): clips and widths around them
    take different paths through it."""
    r, c = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().mgx_hpss_tile(ctypes.byref(r), ctypes.byref(c))
    return int(r.value), int(c.value)


def chroma_params(**params):
    """A ChromaParams with the library's defaults (mgx_chroma_params_init) and `params` over them; numbers out of
    range pass through: the library refuses them with its message."""
    for k in params:
        if k not in CHROMA_PARAMS:
            raise TypeError("chroma parameter %r: one of %s" % (k, ", ".join(CHROMA_PARAMS)))
    p = ChromaParams()
    lib().mgx_chroma_params_init(ctypes.byref(p))
    for k, v in params.items():
        setattr(p, k, int(v) if k in ("num_chroma", "base_c") else float(v))
    return p


def _chroma_norm(norm):
    if isinstance(norm, str):
        if norm not in CHROMA_NORMS:
            raise ValueError("chroma norm %r: one of %s" % (norm, sorted(CHROMA_NORMS)))
        return CHROMA_NORMS[norm]
    return int(norm)


class HostTables(ctypes.Structure):
    _fields_ = [("window", ctypes.c_void_p), ("hanning", ctypes.c_void_p),
                ("hamming", ctypes.c_void_p), ("bark_scale", ctypes.c_void_p),
                ("bark_limits", ctypes.c_void_p), ("mel_bins", ctypes.c_void_p),
                ("dct", ctypes.c_void_p)]


class WavInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("pcm_format", ctypes.c_uint32),
                ("channels", ctypes.c_uint32), ("sample_rate", ctypes.c_uint32),
                ("bits_per_sample", ctypes.c_uint32), ("block_align", ctypes.c_uint32),
                ("data_offset", ctypes.c_uint64), ("data_bytes", ctypes.c_uint64),
                ("sample_frames", ctypes.c_uint64)]


_lib = None


def lib():
    """Load libmeyda_gpu.so (fails loudly if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libmeyda_gpu.so not built (run `make` or __graft_entry__.build())")
        # torch ships its own libamdhip64 (SONAME libamdhip64.so.7). Load it first so
        # the loader resolves our DT_NEEDED libamdhip64.so.7 to that same runtime:
        # two HIP runtimes in one process leave the second without devices.
        try:
            import torch  # noqa: F401
            # multi-device groups load RCCL at run time: in a torch process use torch's own
            # librccl (built against the HIP runtime this process runs on)
            trccl = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
            if "MGX_RCCL_LIB" not in os.environ and os.path.exists(trccl):
                os.environ["MGX_RCCL_LIB"] = trccl
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        L.mgx_plan_desc_init.argtypes = [ctypes.POINTER(PlanDesc)]
        L.mgx_plan_desc_init.restype = None
        L.mgx_plan_create.argtypes = [ctypes.POINTER(PlanDesc), ctypes.POINTER(ctypes.c_void_p)]
        L.mgx_plan_destroy.argtypes = [ctypes.c_void_p]
        L.mgx_plan_get_desc.argtypes = [ctypes.c_void_p, ctypes.POINTER(PlanDesc)]
        L.mgx_extract_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.POINTER(Outputs), ctypes.c_void_p]
        L.mgx_extract_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.POINTER(Outputs)]
        L.mgx_synth_frames_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                              ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        L.mgx_get_host_tables.argtypes = [ctypes.POINTER(PlanDesc), ctypes.POINTER(HostTables)]
        L.mgx_is_power_of_two.argtypes = [ctypes.c_double]
        L.mgx_feature_index.argtypes = [ctypes.c_char_p]
        L.mgx_feature_name.argtypes = [ctypes.c_int]
        L.mgx_feature_name.restype = ctypes.c_char_p
        L.mgx_feature_info.argtypes = [ctypes.c_int]
        L.mgx_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.mgx_last_error.restype = ctypes.c_char_p
        L.mgx_wav_parse.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(WavInfo)]
        L.mgx_pcm_decode_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.mgx_extract_host_pcm.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                           ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Outputs)]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        L.mgx_signal_frames.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p]
        L.mgx_extract_signal_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                                ctypes.POINTER(Outputs), ctypes.c_void_p]
        L.mgx_extract_signal_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                              ctypes.POINTER(Outputs)]
        L.mgx_extract_signal_host_pcm.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                  ctypes.POINTER(Outputs)]
        aux = ctypes.POINTER(AuxOutputs)
        L.mgx_extract_device_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                            ctypes.POINTER(Outputs), aux, ctypes.c_void_p]
        L.mgx_extract_host_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                          ctypes.POINTER(Outputs), aux]
        L.mgx_extract_host_pcm_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                              ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.POINTER(Outputs), aux]
        L.mgx_signals_frame_starts.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, u64p]
        L.mgx_extract_gather_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_uint64, ctypes.POINTER(Outputs), aux, ctypes.c_void_p]
        L.mgx_extract_gather_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                              ctypes.c_uint64, ctypes.POINTER(Outputs), aux]
        summ = ctypes.POINTER(SummaryOutputs)
        L.mgx_summary_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.POINTER(Outputs), aux, summ, ctypes.c_uint64,
                                                  ctypes.c_uint64, u64p]
        L.mgx_summarize_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(Outputs), aux, summ,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.mgx_summarize_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(Outputs), aux, summ]
        dsum = ctypes.POINTER(DeltaSummaries)
        L.mgx_delta_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                       ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.mgx_summarize_deltas_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.POINTER(Outputs), aux, summ, dsum,
                                                           ctypes.c_uint64, ctypes.c_uint64, u64p]
        L.mgx_summarize_deltas_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(Outputs), aux,
                                                  summ, dsum, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.mgx_summarize_deltas_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(Outputs), aux,
                                                summ, dsum]
        freq = ctypes.POINTER(FluxRequest)
        L.mgx_flux_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                      ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.mgx_summarize_flux_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.POINTER(Outputs), aux, summ, dsum, freq,
                                                         ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, u64p]
        L.mgx_summarize_flux_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(Outputs), aux,
                                                summ, dsum, freq, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.mgx_summarize_flux_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                              ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(Outputs), aux,
                                              summ, dsum, freq, ctypes.c_uint32]
        L.mgx_peaks_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, u64p]
        L.mgx_peaks_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.POINTER(PeakParams), ctypes.POINTER(PeakOutputs), ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.c_void_p]
        L.mgx_onsets_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_uint64, freq, ctypes.POINTER(PeakParams), ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_uint64]
        L.mgx_hpss_params_init.argtypes = [ctypes.POINTER(HpssParams)]
        L.mgx_hpss_params_init.restype = None
        L.mgx_hpss_tile.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.mgx_hpss_tile.restype = None
        L.mgx_hpss_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.POINTER(HpssParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.mgx_hpss_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                    ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HpssParams), ctypes.POINTER(ChromaRequest),
                                    ctypes.POINTER(FluxRequest), ctypes.c_void_p, ctypes.c_void_p]
        L.mgx_chroma_params_init.argtypes = [ctypes.POINTER(ChromaParams)]
        L.mgx_chroma_params_init.restype = None
        L.mgx_chroma_weights.argtypes = [ctypes.c_uint32, ctypes.c_double, ctypes.POINTER(ChromaParams), ctypes.c_void_p]
        L.mgx_chroma_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.mgx_chroma_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ChromaRequest)]
        tpar = ctypes.POINTER(TempoParams)
        L.mgx_tempo_params_init.argtypes = [tpar]
        L.mgx_tempo_params_init.restype = None
        L.mgx_tempogram_window.argtypes = [ctypes.c_uint32, ctypes.c_void_p]
        L.mgx_tempo_prior.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_uint32,
                                      ctypes.c_void_p]
        L.mgx_tempogram_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                           ctypes.c_void_p]
        L.mgx_tempo_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, tpar, ctypes.c_uint32, u64p]
        L.mgx_tempo_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, tpar,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.mgx_tempo_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.c_void_p, ctypes.c_uint64, freq, tpar, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]
        bpar = ctypes.POINTER(BeatParams)
        L.mgx_beat_params_init.argtypes = [bpar]
        L.mgx_beat_params_init.restype = None
        L.mgx_beat_tables.argtypes = [ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        L.mgx_beats_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, u64p]
        L.mgx_beats_device.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.c_void_p, bpar, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.POINTER(PeakOutputs), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.mgx_beats_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.c_void_p, ctypes.c_uint64, freq, tpar, ctypes.c_void_p, ctypes.c_void_p, bpar,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_uint64]
        L.mgx_shard_range.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p, u64p]
        L.mgx_packed_layout.argtypes = [ctypes.POINTER(PlanDesc), ctypes.c_uint32, ctypes.c_uint64, u64p]
        L.mgx_packed_layout.restype = ctypes.c_uint64
        L.mgx_comm_unique_id.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        L.mgx_group_create.argtypes = [ctypes.POINTER(PlanDesc), ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32,
                                       ctypes.POINTER(ctypes.c_void_p)]
        L.mgx_group_create_rank.argtypes = [ctypes.POINTER(PlanDesc), ctypes.c_void_p, ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
        L.mgx_group_create_loopback.argtypes = [ctypes.POINTER(PlanDesc), ctypes.c_uint32,
                                                ctypes.POINTER(ctypes.c_void_p)]
        L.mgx_group_create_loopback_rccl.argtypes = [ctypes.POINTER(PlanDesc), ctypes.c_uint32,
                                                     ctypes.POINTER(ctypes.c_void_p)]
        L.mgx_group_destroy.argtypes = [ctypes.c_void_p]
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.mgx_group_comm_info.argtypes = [ctypes.c_void_p, i32p, i32p, i32p]
        L.mgx_group_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                     ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.mgx_group_extract_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), u64p,
                                               ctypes.POINTER(Outputs), ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.POINTER(ctypes.c_void_p)]
        L.mgx_group_extract_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.POINTER(Outputs)]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise MgxError(rc, lib().mgx_last_error().decode())
    return rc


def make_desc(buffer_size=512, sample_rate=44100.0, window="hanning", precision="faithful",
              mode="per_buffer_fft", num_mel_bands=26, num_mfcc_coeffs=13, scalar_f64=False,
              device=0, dct_sequential=False, mfcc_reference=False, resident=False):
    d = PlanDesc()
    lib().mgx_plan_desc_init(ctypes.byref(d))
    d.buffer_size = buffer_size
    d.sample_rate = sample_rate
    d.window = WINDOWS[window]
    d.precision = PRECISIONS[precision]
    d.mode = MODES[mode]
    d.num_mel_bands = num_mel_bands
    d.num_mfcc_coeffs = num_mfcc_coeffs
    d.scalar_f64 = 1 if scalar_f64 else 0
    d.device = device
    d.flags = ((FLAG_DCT_SEQUENTIAL if dct_sequential else 0) | (FLAG_MFCC_REFERENCE if mfcc_reference else 0) |
               (FLAG_RESIDENT if resident else 0))
    return d


def host_tables(**kw):
    """Host tables (window, bark, limits, mel bins, dct) computed by the library: no GPU."""
    d = make_desc(**kw)
    n, nf, nc = d.buffer_size, d.num_mel_bands, d.num_mfcc_coeffs
    t = {"window": np.empty(n, np.float32), "hanning": np.empty(n, np.float32),
         "hamming": np.empty(n, np.float32), "bark_scale": np.empty(n, np.float32),
         "bark_limits": np.empty(NUM_BARK + 1, np.int32), "mel_bins": np.empty(nf + 2, np.int32),
         "dct": np.empty(nc * nf, np.float32)}
    ht = HostTables(*[t[k].ctypes.data for k in ("window", "hanning", "hamming", "bark_scale",
                                                  "bark_limits", "mel_bins", "dct")])
    check(lib().mgx_get_host_tables(ctypes.byref(d), ctypes.byref(ht)))
    return t


def signal_frames(num_samples, n, hop):
    """Buffers of `n` samples, `hop` apart, in a signal of `num_samples` (mgx_signal_frames; host only)."""
    f = ctypes.c_uint64()
    check(lib().mgx_signal_frames(num_samples, n, hop, ctypes.byref(f)))
    return f.value


def signals_frame_starts(lengths_or_offsets, n, hop, offsets=False):
    """The buffers of several signals stored one after another (mgx_signals_frame_starts; host only): `n`
    samples each, `hop` apart within a signal, none across a signal's end. lengths_or_offsets: the signals'
    lengths, or with offsets=True their num_signals + 1 offsets into the concatenated array. Returns
    (starts, frame_offsets), uint64 arrays: the start of every buffer in signal order, and the
    num_signals + 1 prefix sums of the signals' buffer counts."""
    v = np.asarray(lengths_or_offsets, dtype=np.uint64).ravel()
    off = np.ascontiguousarray(v) if offsets else np.concatenate([np.zeros(1, np.uint64), np.cumsum(v, dtype=np.uint64)])
    ns = off.size - 1
    total = ctypes.c_uint64()
    check(lib().mgx_signals_frame_starts(off.ctypes.data, ns, n, hop, None, None, 0, ctypes.byref(total)))
    starts, frame_offsets = np.empty(total.value, np.uint64), np.empty(ns + 1, np.uint64)
    check(lib().mgx_signals_frame_starts(off.ctypes.data, ns, n, hop, frame_offsets.ctypes.data, starts.ctypes.data,
                                         starts.size, ctypes.byref(total)))
    return starts, frame_offsets


def device_count():
    c = ctypes.c_int(0)
    check(lib().mgx_device_count(ctypes.byref(c)))
    return c.value


class Plan:
    """One extraction plan (mirrors `new Meyda(ctx, src, bufferSize)`, src/meyda.js:17-97)."""

    def __init__(self, buffer_size=512, **kw):
        self.desc = make_desc(buffer_size=buffer_size, **kw)
        h = ctypes.c_void_p()
        check(lib().mgx_plan_create(ctypes.byref(self.desc), ctypes.byref(h)))
        self._h = h
        self.n = buffer_size
        self.scalar_dtype = np.float64 if kw.get("scalar_f64") else np.float32

    def close(self):
        if getattr(self, "_h", None):
            lib().mgx_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------- device (torch)
    def alloc_outputs(self, num_frames, features, device="cuda"):
        """Allocate torch device tensors for the requested features; returns (dict, Outputs). "melBands" (an
        output beyond mgx_outputs) rides on the Outputs as its `aux` attribute, an AuxOutputs: the extract
        methods below then make the mgx_extract_*_ex call."""
        import torch
        st = torch.float64 if self.scalar_dtype == np.float64 else torch.float32
        L = self.n // 2
        out, o = {}, Outputs()
        for f in features:
            if f in SCALAR_NAMES:
                out[f] = torch.empty(num_frames, dtype=st, device=device)
                o.scalars[SCALAR_NAMES.index(f)] = out[f].data_ptr()
            elif f == "loudness":
                out["loudness.specific"] = torch.empty(num_frames, NUM_BARK, dtype=torch.float32, device=device)
                o.loudness_specific = out["loudness.specific"].data_ptr()
                out["loudness.total"] = torch.empty(num_frames, dtype=st, device=device)
                o.scalars[10] = out["loudness.total"].data_ptr()
            elif f == "mfcc":
                out[f] = torch.empty(num_frames, self.desc.num_mfcc_coeffs, dtype=torch.float32, device=device)
                o.mfcc = out[f].data_ptr()
            elif f == "melBands":
                out[f] = torch.empty(num_frames, self.desc.num_mel_bands, dtype=torch.float32, device=device)
                _set_mel_bands(o, out[f].data_ptr())
            elif f == "amplitudeSpectrum":
                out[f] = torch.empty(num_frames, L, dtype=torch.float32, device=device)
                o.amplitude_spectrum = out[f].data_ptr()
            elif f == "powerSpectrum":
                out[f] = torch.empty(num_frames, L, dtype=torch.float32, device=device)
                o.power_spectrum = out[f].data_ptr()
            elif f == "complexSpectrum":
                out["complexSpectrum.real"] = torch.empty(num_frames, self.n, dtype=torch.float32, device=device)
                out["complexSpectrum.imag"] = torch.empty(num_frames, self.n, dtype=torch.float32, device=device)
                o.complex_real = out["complexSpectrum.real"].data_ptr()
                o.complex_imag = out["complexSpectrum.imag"].data_ptr()
            else:
                raise ValueError("unknown feature %r" % f)
        return out, o

    def extract_device(self, frames_ptr, num_frames, outputs, stream=None):
        """Launch on device pointers (async on `stream`, an int hipStream_t handle or None)."""
        if _aux(outputs) is not None:  # the dense batch as a signal at hop N (the same launch, bit for bit)
            return self.extract_signal_device(frames_ptr, num_frames * self.n, self.n, outputs, stream)
        check(lib().mgx_extract_device(self._h, ctypes.c_void_p(frames_ptr), num_frames,
                                       ctypes.byref(outputs), ctypes.c_void_p(stream or 0)))

    def extract_torch(self, frames, features, stream=None):
        """frames: a (F, N) float32 CUDA tensor. Returns a dict of device tensors."""
        import torch
        assert frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous()
        assert frames.dim() == 2 and frames.shape[1] == self.n
        out, o = self.alloc_outputs(frames.shape[0], features, device=frames.device)
        if stream is None:
            stream = torch.cuda.current_stream(frames.device).cuda_stream
        self.extract_device(frames.data_ptr(), frames.shape[0], o, stream)
        return out

    def extract_signal_device(self, samples_ptr, num_samples, hop, outputs, stream=None):
        """Launch on a device signal cut every `hop` samples (async; outputs sized for signal_frames())."""
        if _aux(outputs) is not None:
            check(lib().mgx_extract_device_ex(self._h, ctypes.c_void_p(samples_ptr), num_samples, hop,
                                              ctypes.byref(outputs), _aux_ref(outputs), ctypes.c_void_p(stream or 0)))
            return
        check(lib().mgx_extract_signal_device(self._h, ctypes.c_void_p(samples_ptr), num_samples, hop,
                                              ctypes.byref(outputs), ctypes.c_void_p(stream or 0)))

    def extract_signal_torch(self, samples, hop, features, stream=None):
        """samples: a 1-D float32 CUDA tensor (any 4-byte alignment). Returns a dict of device tensors over
        the signal_frames(len(samples), N, hop) overlapping buffers; the buffers are not materialised."""
        import torch
        assert samples.is_cuda and samples.dtype == torch.float32 and samples.is_contiguous() and samples.dim() == 1
        S = samples.shape[0]
        out, o = self.alloc_outputs(signal_frames(S, self.n, hop), features, device=samples.device)
        if stream is None:
            stream = torch.cuda.current_stream(samples.device).cuda_stream
        self.extract_signal_device(samples.data_ptr(), S, hop, o, stream)
        return out

    def extract_gather_device(self, samples_ptr, num_samples, starts_ptr, num_frames, outputs, stream=None):
        """Launch on device pointers: buffer f is samples [starts[f], starts[f] + N) (uint64 starts; async)."""
        check(lib().mgx_extract_gather_device(self._h, ctypes.c_void_p(samples_ptr), num_samples, ctypes.c_void_p(starts_ptr),
                                              num_frames, ctypes.byref(outputs), _aux_ref(outputs),
                                              ctypes.c_void_p(stream or 0)))

    def extract_gather_torch(self, samples, starts, features, stream=None):
        """samples: a 1-D float32 CUDA tensor (any 4-byte alignment); starts: a 1-D int64 CUDA tensor of
        non-negative sample indices (read as the ABI's uint64), or anything numpy turns into one. Returns a
        dict of device tensors over the len(starts) buffers; the buffers are not materialised."""
        import torch
        assert samples.is_cuda and samples.dtype == torch.float32 and samples.is_contiguous() and samples.dim() == 1
        if not torch.is_tensor(starts):
            starts = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint64).view(np.int64)).to(samples.device)
        assert starts.is_cuda and starts.dtype == torch.int64 and starts.is_contiguous() and starts.dim() == 1
        out, o = self.alloc_outputs(starts.shape[0], features, device=samples.device)
        if stream is None:
            stream = torch.cuda.current_stream(samples.device).cuda_stream
        self.extract_gather_device(samples.data_ptr(), samples.shape[0], starts.data_ptr(), starts.shape[0], o, stream)
        # (the launch reads the table: a caller who passes a stream other than torch's current one keeps
        # `starts` alive until the launch has ended, as it does `samples`)
        return out

    # ------------------------------------------------------------------ host
    def extract_gather(self, samples, starts, features):
        """Host numpy signal and starts in / numpy out: buffer f is samples [starts[f], starts[f] + N)."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        assert samples.ndim == 1 and starts.ndim == 1
        out, o = self._host_outputs(starts.size, features)
        check(lib().mgx_extract_gather_host(self._h, samples.ctypes.data, samples.size, starts.ctypes.data, starts.size,
                                            ctypes.byref(o), _aux_ref(o)))
        return out

    def extract_signals(self, signals, hop, features):
        """A list of 1-D host signals in one call: every signal's buffers, `hop` apart, none across two signals.
        Returns (outputs, frame_offsets): signal s's rows of every output are
        [frame_offsets[s], frame_offsets[s + 1])."""
        signals = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in signals]
        starts, frame_offsets = signals_frame_starts([x.size for x in signals], self.n, hop)
        samples = np.concatenate(signals) if signals else np.empty(0, np.float32)
        return self.extract_gather(samples, starts, features), frame_offsets

    # ------------------------------------------------------- per-signal summaries
    def _summary_outputs(self, S, features, alloc):
        """A SummaryOutputs over arrays alloc(shape) (float64; .data_ptr() or .ctypes.data), and the arrays by
        name: (S, 4, width) each, statistic k of signal s at [s, k] (STATS). "loudness" pools specific and total."""
        widths = {"loudness.specific": NUM_BARK, "mfcc": self.desc.num_mfcc_coeffs, "amplitudeSpectrum": self.n // 2,
                  "powerSpectrum": self.n // 2, "melBands": self.desc.num_mel_bands}
        slots = {"loudness.specific": "loudness_specific", "mfcc": "mfcc", "amplitudeSpectrum": "amplitude_spectrum",
                 "powerSpectrum": "power_spectrum", "melBands": "mel_bands"}
        so = SummaryOutputs()
        so.struct_size = ctypes.sizeof(SummaryOutputs)
        out = {}
        for f in features:
            if f not in SUMMARY_FEATURES:
                raise ValueError("%r has no summary" % (f,))
            for name in (["loudness.specific", "loudness.total"] if f == "loudness" else [f]):
                arr = alloc((S, len(STATS), widths.get(name, 1)))
                out[name] = arr
                ptr = arr.data_ptr() if hasattr(arr, "data_ptr") else arr.ctypes.data
                if name in SCALAR_NAMES:
                    so.scalars[SCALAR_NAMES.index(name)] = ptr
                else:
                    setattr(so, slots[name], ptr)
        return out, so

    def summary_workspace_bytes(self, outputs, summary, num_frames, num_signals):
        """mgx_summary_workspace_bytes (host only): the device workspace of summarize_device with these arguments."""
        b = ctypes.c_uint64()
        check(lib().mgx_summary_workspace_bytes(self._h, ctypes.byref(outputs), _aux_ref(outputs), ctypes.byref(summary),
                                                num_frames, num_signals, ctypes.byref(b)))
        return b.value

    def summarize_device(self, samples_ptr, num_samples, starts_ptr, num_frames, offsets_ptr, num_signals, outputs, summary,
                         workspace_ptr, workspace_bytes, stream=None):
        """mgx_summarize_device on device pointers (async on `stream`)."""
        check(lib().mgx_summarize_device(self._h, ctypes.c_void_p(samples_ptr), num_samples, ctypes.c_void_p(starts_ptr),
                                         num_frames, ctypes.c_void_p(offsets_ptr), num_signals, ctypes.byref(outputs),
                                         _aux_ref(outputs), ctypes.byref(summary), ctypes.c_void_p(workspace_ptr),
                                         workspace_bytes, ctypes.c_void_p(stream or 0)))

    def _delta_summaries(self, S, features, deltas, alloc):
        """deltas = (width, order): a DeltaSummaries over arrays alloc(shape) for the delta (and at order 2 the
        second-order) rows of `features`, and the arrays by name as _summary_outputs gives them (None at order 1
        for the second). Spectrum features pass through: the library refuses them with its own message."""
        width, order = deltas
        if order not in (1, 2):
            raise ValueError("delta order %r: 1 or 2" % (order,))
        d1, so1 = self._summary_outputs(S, features, alloc)
        d2, so2 = self._summary_outputs(S, features, alloc) if order == 2 else (None, None)
        ds = DeltaSummaries()
        ds.struct_size = ctypes.sizeof(DeltaSummaries)
        ds.width = width
        ds.delta = ctypes.pointer(so1)
        if so2 is not None:
            ds.delta2 = ctypes.pointer(so2)
        ds.keep = (so1, so2)  # (the structs the pointers name live as long as this one)
        return d1, d2, ds

    def summarize_deltas_workspace_bytes(self, outputs, summary, deltas, num_frames, num_signals):
        """mgx_summarize_deltas_workspace_bytes (host only); deltas: a DeltaSummaries or None."""
        b = ctypes.c_uint64()
        check(lib().mgx_summarize_deltas_workspace_bytes(self._h, ctypes.byref(outputs), _aux_ref(outputs), ctypes.byref(summary),
                                                         None if deltas is None else ctypes.byref(deltas), num_frames,
                                                         num_signals, ctypes.byref(b)))
        return b.value

    def summarize_deltas_device(self, samples_ptr, num_samples, starts_ptr, num_frames, offsets_ptr, num_signals, outputs,
                                summary, deltas, workspace_ptr, workspace_bytes, stream=None):
        """mgx_summarize_deltas_device on device pointers (async on `stream`); deltas: a DeltaSummaries or None."""
        check(lib().mgx_summarize_deltas_device(self._h, ctypes.c_void_p(samples_ptr), num_samples, ctypes.c_void_p(starts_ptr),
                                                num_frames, ctypes.c_void_p(offsets_ptr), num_signals, ctypes.byref(outputs),
                                                _aux_ref(outputs), ctypes.byref(summary),
                                                None if deltas is None else ctypes.byref(deltas),
                                                ctypes.c_void_p(workspace_ptr), workspace_bytes, ctypes.c_void_p(stream or 0)))

    def _flux_requests(self, F, S, flux, alloc, alloc32):
        """flux: a list of dicts {feature, mode ("rectified", "l1", "l2" or its number; default "rectified"), lag
        (default 1), per_frame (default False), summary (default True)}. Returns the array of FluxRequest over
        arrays alloc((S, 4)) (float64) and alloc32((F,)) (float32), and the results: one dict per request with
        "feature", "mode", "lag", "summary" ((S, 4): mean, variance, min, max of the flux per signal, or None) and
        "per_frame" ((F,), or None). Numbers out of range pass through: the library refuses them with its message."""
        reqs = (FluxRequest * max(len(flux), 1))()
        ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
        out = []
        for i, f in enumerate(flux):
            name = f["feature"]
            if name not in FLUX_FEATURES:
                raise ValueError("%r has no flux" % (name,))
            mode = f.get("mode", "rectified")
            if isinstance(mode, str):
                if mode not in FLUX_MODES:
                    raise ValueError("flux mode %r: one of %s" % (mode, sorted(FLUX_MODES)))
                mode = FLUX_MODES[mode]
            res = {"feature": name, "mode": mode, "lag": f.get("lag", 1), "summary": None, "per_frame": None}
            r = reqs[i]
            r.struct_size = ctypes.sizeof(FluxRequest)
            r.field, r.mode, r.lag = FLUX_FEATURES[name], mode, res["lag"]
            if f.get("summary", True):
                res["summary"] = alloc((S, len(STATS)))
                r.summary = ptr(res["summary"])
            if f.get("per_frame", False):
                res["per_frame"] = alloc32((F,))
                r.per_frame = ptr(res["per_frame"])
            out.append(res)
        return reqs, out

    def summarize_flux_workspace_bytes(self, outputs, summary, deltas, flux, num_flux, num_frames, num_signals):
        """mgx_summarize_flux_workspace_bytes (host only); deltas: a DeltaSummaries or None; flux: a FluxRequest array."""
        b = ctypes.c_uint64()
        check(lib().mgx_summarize_flux_workspace_bytes(self._h, ctypes.byref(outputs), _aux_ref(outputs), ctypes.byref(summary),
                                                       None if deltas is None else ctypes.byref(deltas), flux, num_flux,
                                                       num_frames, num_signals, ctypes.byref(b)))
        return b.value

    def summarize_flux_device(self, samples_ptr, num_samples, starts_ptr, num_frames, offsets_ptr, num_signals, outputs,
                              summary, deltas, flux, num_flux, workspace_ptr, workspace_bytes, stream=None):
        """mgx_summarize_flux_device on device pointers (async on `stream`)."""
        check(lib().mgx_summarize_flux_device(self._h, ctypes.c_void_p(samples_ptr), num_samples, ctypes.c_void_p(starts_ptr),
                                              num_frames, ctypes.c_void_p(offsets_ptr), num_signals, ctypes.byref(outputs),
                                              _aux_ref(outputs), ctypes.byref(summary),
                                              None if deltas is None else ctypes.byref(deltas), flux, num_flux,
                                              ctypes.c_void_p(workspace_ptr), workspace_bytes, ctypes.c_void_p(stream or 0)))

    def summarize_gather_torch(self, samples, starts, frame_offsets, features, per_frame=(), stream=None, deltas=None, flux=None):
        """extract_gather_torch with every signal's rows pooled on the device: signal s owns rows
        [frame_offsets[s], frame_offsets[s + 1]) (int64 CUDA tensors, or anything numpy turns into one). Returns
        (summaries, rows): per pooled field a float64 CUDA tensor (S, 4, width) of mean, variance, min, max, and
        the per-frame tensors of the features named in `per_frame`. The workspace is allocated here and handed to
        torch's allocator again when this returns, which orders its reuse after the launch on torch's current
        stream: a caller who passes another stream synchronises it before allocating again.
        deltas = (width, order): the rows' regression deltas of that half-width are pooled too
        (mgx_summarize_deltas_device), and the result is (summaries, rows, delta_summaries, delta2_summaries), the
        last None at order 1.
        flux = a list of requests (_flux_requests): the flux of those fields per frame and pooled
        (mgx_summarize_flux_device); the result then has one more element, the list of the requests' results
        (a per_frame column is zero in rows that belong to no signal)."""
        import torch
        assert samples.is_cuda and samples.dtype == torch.float32 and samples.is_contiguous() and samples.dim() == 1
        dev = samples.device

        def table(v):
            if not torch.is_tensor(v):
                v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint64).view(np.int64)).to(dev)
            assert v.is_cuda and v.dtype == torch.int64 and v.is_contiguous() and v.dim() == 1
            return v
        starts, frame_offsets = table(starts), table(frame_offsets)
        F, S = starts.shape[0], frame_offsets.shape[0] - 1
        rows, o = self.alloc_outputs(F, per_frame, device=dev)
        summ, so = self._summary_outputs(S, features, lambda shape: torch.empty(shape, dtype=torch.float64, device=dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        if flux is not None:
            d1 = d2 = ds = None
            if deltas is not None:
                d1, d2, ds = self._delta_summaries(S, features, deltas,
                                                   lambda shape: torch.empty(shape, dtype=torch.float64, device=dev))
            reqs, fres = self._flux_requests(F, S, flux, lambda shape: torch.empty(shape, dtype=torch.float64, device=dev),
                                             lambda shape: torch.zeros(shape, dtype=torch.float32, device=dev))
            nbytes = self.summarize_flux_workspace_bytes(o, so, ds, reqs, len(flux), F, S)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            self.summarize_flux_device(samples.data_ptr(), samples.shape[0], starts.data_ptr(), F, frame_offsets.data_ptr(), S,
                                       o, so, ds, reqs, len(flux), ws.data_ptr(), nbytes, stream)
            return (summ, rows, d1, d2, fres) if deltas is not None else (summ, rows, fres)
        if deltas is not None:
            d1, d2, ds = self._delta_summaries(S, features, deltas,
                                               lambda shape: torch.empty(shape, dtype=torch.float64, device=dev))
            nbytes = self.summarize_deltas_workspace_bytes(o, so, ds, F, S)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            self.summarize_deltas_device(samples.data_ptr(), samples.shape[0], starts.data_ptr(), F, frame_offsets.data_ptr(), S,
                                         o, so, ds, ws.data_ptr(), nbytes, stream)
            return summ, rows, d1, d2
        nbytes = self.summary_workspace_bytes(o, so, F, S)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        self.summarize_device(samples.data_ptr(), samples.shape[0], starts.data_ptr(), F, frame_offsets.data_ptr(), S, o, so,
                              ws.data_ptr(), nbytes, stream)
        return summ, rows

    def summarize_gather(self, samples, starts, frame_offsets, features, per_frame=(), deltas=None, flux=None):
        """Host numpy in / numpy out (mgx_summarize_host): (summaries, rows) as summarize_gather_torch gives them;
        with deltas = (width, order) (mgx_summarize_deltas_host), (summaries, rows, delta_summaries, delta2_summaries);
        with flux = a list of requests (mgx_summarize_flux_host), one more element: the requests' results."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        frame_offsets = np.ascontiguousarray(frame_offsets, dtype=np.uint64)
        assert samples.ndim == 1 and starts.ndim == 1 and frame_offsets.ndim == 1 and frame_offsets.size >= 1
        S = frame_offsets.size - 1
        rows, o = self._host_outputs(starts.size, per_frame)
        summ, so = self._summary_outputs(S, features, lambda shape: np.empty(shape, np.float64))
        if flux is not None:
            d1 = d2 = ds = None
            if deltas is not None:
                d1, d2, ds = self._delta_summaries(S, features, deltas, lambda shape: np.empty(shape, np.float64))
            reqs, fres = self._flux_requests(starts.size, S, flux, lambda shape: np.empty(shape, np.float64),
                                             lambda shape: np.zeros(shape, np.float32))
            check(lib().mgx_summarize_flux_host(self._h, samples.ctypes.data, samples.size, starts.ctypes.data, starts.size,
                                                frame_offsets.ctypes.data, S, ctypes.byref(o), _aux_ref(o), ctypes.byref(so),
                                                None if ds is None else ctypes.byref(ds), reqs, len(flux)))
            return (summ, rows, d1, d2, fres) if deltas is not None else (summ, rows, fres)
        if deltas is not None:
            d1, d2, ds = self._delta_summaries(S, features, deltas, lambda shape: np.empty(shape, np.float64))
            check(lib().mgx_summarize_deltas_host(self._h, samples.ctypes.data, samples.size, starts.ctypes.data, starts.size,
                                                  frame_offsets.ctypes.data, S, ctypes.byref(o), _aux_ref(o), ctypes.byref(so),
                                                  ctypes.byref(ds)))
            return summ, rows, d1, d2
        check(lib().mgx_summarize_host(self._h, samples.ctypes.data, samples.size, starts.ctypes.data, starts.size,
                                       frame_offsets.ctypes.data, S, ctypes.byref(o), _aux_ref(o), ctypes.byref(so)))
        return summ, rows

    def onsets(self, samples, starts, frame_offsets, feature="melBands", mode="rectified", lag=1, envelope=False, summary=False,
               capacity=None, **params):
        """Host numpy in / numpy out (mgx_onsets_host): the flux of `feature` over the buffers at `starts`, and its
        peaks within each signal picked on the device (params: pre_max, post_max, pre_avg, post_avg, delta, wait).
        Returns a dict: "peak_offsets" (S + 1, uint64: the true counts), "peaks" (the row indices, ascending; the
        first `capacity` when that is given and smaller, None with capacity 0), and "envelope" ((F,) float32, zero
        in rows of no signal) and "summary" ((S, 4)) when asked. Without `capacity` the call is made twice: once for
        the counts, once for the list."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        frame_offsets = np.ascontiguousarray(frame_offsets, dtype=np.uint64)
        assert samples.ndim == 1 and starts.ndim == 1 and frame_offsets.ndim == 1 and frame_offsets.size >= 1
        S = frame_offsets.size - 1
        req = {"feature": feature, "mode": mode, "lag": lag, "per_frame": envelope, "summary": summary}
        reqs, fres = self._flux_requests(starts.size, S, [req], lambda shape: np.empty(shape, np.float64),
                                         lambda shape: np.zeros(shape, np.float32))
        pp = peak_params(**params)
        offsets = np.zeros(S + 1, np.uint64)

        def call(peaks, cap):
            check(lib().mgx_onsets_host(self._h, samples.ctypes.data, samples.size, starts.ctypes.data, starts.size,
                                        frame_offsets.ctypes.data, S, reqs, ctypes.byref(pp), offsets.ctypes.data,
                                        None if peaks is None else peaks.ctypes.data, cap))
        peaks = None
        if capacity is None or capacity == 0:
            call(None, 0)
            if capacity is None:
                capacity, peaks = int(offsets[S]), np.zeros(0, np.uint64)
        if capacity > 0:
            peaks = np.zeros(capacity, np.uint64)
            call(peaks, capacity)
            peaks = peaks[:min(capacity, int(offsets[S]))]
        res = {"peak_offsets": offsets, "peaks": peaks}
        if envelope:
            res["envelope"] = fres[0]["per_frame"]
        if summary:
            res["summary"] = fres[0]["summary"]
        return res

    def tempo(self, samples, starts, frame_offsets, frame_rate, feature="melBands", mode="rectified", lag=1, win_length=384,
              num_lags=None, norm="lag0", gain=1e6, start_bpm=120.0, std_octaves=1.0, max_bpm=320.0, window=None, prior=None,
              mean=False, envelope=False, envelope_summary=False):
        """Host numpy in / numpy out (mgx_tempo_host): the flux of `feature` over the buffers at `starts`, its
        autocorrelation tempogram (window: W float32, None: tempogram_window) pooled per signal, and the lag the
        prior picks (prior: L float64, None: tempo_prior of frame_rate, the rows per second, with start_bpm,
        std_octaves, max_bpm). Returns a dict: "lag" ((S,) uint32, 0: none), "bpm" ((S,) float64, 60 frame_rate /
        lag, NaN where the lag is 0), "window", "prior", and when asked "summary" ((S, 4, L) float64: mean, variance,
        min, max of the tempogram rows per signal; `mean`), "envelope" ((F,) float32) and "envelope_summary" ((S, 4))."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        frame_offsets = np.ascontiguousarray(frame_offsets, dtype=np.uint64)
        assert samples.ndim == 1 and starts.ndim == 1 and frame_offsets.ndim == 1 and frame_offsets.size >= 1
        S = frame_offsets.size - 1
        tp = tempo_params(win_length, num_lags, norm, gain)
        W, L = int(tp.win_length), int(tp.num_lags)
        window = tempogram_window(W) if window is None else np.ascontiguousarray(window, dtype=np.float32)
        prior = tempo_prior(frame_rate, L, start_bpm, std_octaves, max_bpm) if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
        assert window.shape == (W,) and prior.shape == (L,)
        req = {"feature": feature, "mode": mode, "lag": lag, "per_frame": envelope, "summary": envelope_summary}
        reqs, fres = self._flux_requests(starts.size, S, [req], lambda shape: np.empty(shape, np.float64),
                                         lambda shape: np.zeros(shape, np.float32))
        lags = np.zeros(S, np.uint32)
        summ = np.empty((S, len(STATS), L), np.float64) if mean else None
        check(lib().mgx_tempo_host(self._h, samples.ctypes.data, samples.size, starts.ctypes.data, starts.size,
                                   frame_offsets.ctypes.data, S, reqs, ctypes.byref(tp), window.ctypes.data, prior.ctypes.data,
                                   None if summ is None else summ.ctypes.data, lags.ctypes.data))
        res = {"lag": lags, "bpm": lag_bpm(lags, frame_rate), "window": window, "prior": prior}
        if mean:
            res["summary"] = summ
        if envelope:
            res["envelope"] = fres[0]["per_frame"]
        if envelope_summary:
            res["envelope_summary"] = fres[0]["summary"]
        return res

    def tempo_signals(self, signals, hop, frame_rate=None, **kw):
        """A list of 1-D host signals in one call (Plan.tempo over signals_frame_starts of their lengths; frame_rate
        None: the plan's sample rate / hop): the dict Plan.tempo returns, with "frame_offsets"."""
        signals = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in signals]
        starts, frame_offsets = signals_frame_starts([x.size for x in signals], self.n, hop)
        samples = np.concatenate(signals) if signals else np.empty(0, np.float32)
        if frame_rate is None:
            frame_rate = float(self.desc.sample_rate) / hop
        res = self.tempo(samples, starts, frame_offsets, frame_rate, **kw)
        res["frame_offsets"] = frame_offsets
        return res

    def beats(self, samples, starts, frame_offsets, frame_rate, feature="melBands", mode="rectified", lag=1, win_length=384,
              num_lags=None, norm="lag0", gain=1e6, start_bpm=120.0, std_octaves=1.0, max_bpm=320.0, window=None, prior=None,
              tightness=100.0, trim=True, max_period=None, tables=None, envelope=False, envelope_summary=False, capacity=None):
        """Host numpy in / numpy out (mgx_beats_host): Plan.tempo's route -- the flux of `feature`, its tempogram
        pooled per signal, the lag the prior picks -- and the beats of every signal at its lag, tracked on the
        device over the column that never crosses back (tables: (gauss, penalty) of beat_tables(max_period,
        tightness), None: made here; max_period None: num_lags - 1, the largest lag there can be). Returns a dict:
        "lag" and "bpm" as Plan.tempo, "peak_offsets" (S + 1, uint64: the true counts), "beats" (the row indices,
        ascending; the first `capacity` when that is given and smaller, None with capacity 0), and "envelope",
        "envelope_summary" when asked. Without `capacity` the call is made twice: for the counts, then for the list."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        frame_offsets = np.ascontiguousarray(frame_offsets, dtype=np.uint64)
        assert samples.ndim == 1 and starts.ndim == 1 and frame_offsets.ndim == 1 and frame_offsets.size >= 1
        S = frame_offsets.size - 1
        tp = tempo_params(win_length, num_lags, norm, gain)
        W, L = int(tp.win_length), int(tp.num_lags)
        window = tempogram_window(W) if window is None else np.ascontiguousarray(window, dtype=np.float32)
        prior = tempo_prior(frame_rate, L, start_bpm, std_octaves, max_bpm) if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
        assert window.shape == (W,) and prior.shape == (L,)
        bp = beat_params(max(L - 1, 1) if max_period is None else max_period, trim)
        P = int(bp.max_period)
        gauss, penalty = beat_tables(P, tightness) if tables is None else tables
        gauss, penalty = np.ascontiguousarray(gauss, dtype=np.float32), np.ascontiguousarray(penalty, dtype=np.float64)
        if 1 <= P <= BEAT_MAX_PERIOD:
            assert gauss.shape == ((P + 1) * (P + 2) // 2,) and penalty.shape == ((P + 1) ** 2,)
        req = {"feature": feature, "mode": mode, "lag": lag, "per_frame": envelope, "summary": envelope_summary}
        reqs, fres = self._flux_requests(starts.size, S, [req], lambda shape: np.empty(shape, np.float64),
                                         lambda shape: np.zeros(shape, np.float32))
        lags = np.zeros(S, np.uint32)
        offsets = np.zeros(S + 1, np.uint64)

        def call(rows, cap):
            check(lib().mgx_beats_host(self._h, samples.ctypes.data, samples.size, starts.ctypes.data, starts.size,
                                       frame_offsets.ctypes.data, S, reqs, ctypes.byref(tp), window.ctypes.data, prior.ctypes.data,
                                       ctypes.byref(bp), gauss.ctypes.data, penalty.ctypes.data, lags.ctypes.data, offsets.ctypes.data,
                                       None if rows is None else rows.ctypes.data, cap))
        rows = None
        if capacity is None or capacity == 0:
            call(None, 0)
            if capacity is None:
                capacity, rows = int(offsets[S]), np.zeros(0, np.uint64)
        if capacity > 0:
            rows = np.zeros(capacity, np.uint64)
            call(rows, capacity)
            rows = rows[:min(capacity, int(offsets[S]))]
        res = {"lag": lags, "bpm": lag_bpm(lags, frame_rate), "peak_offsets": offsets, "beats": rows, "window": window, "prior": prior}
        if envelope:
            res["envelope"] = fres[0]["per_frame"]
        if envelope_summary:
            res["envelope_summary"] = fres[0]["summary"]
        return res

    def beats_signals(self, signals, hop, frame_rate=None, **kw):
        """A list of 1-D host signals in one call (Plan.beats over signals_frame_starts of their lengths; frame_rate
        None: the plan's sample rate / hop): the dict Plan.beats returns, with "frame_offsets"."""
        signals = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in signals]
        starts, frame_offsets = signals_frame_starts([x.size for x in signals], self.n, hop)
        samples = np.concatenate(signals) if signals else np.empty(0, np.float32)
        if frame_rate is None:
            frame_rate = float(self.desc.sample_rate) / hop
        res = self.beats(samples, starts, frame_offsets, frame_rate, **kw)
        res["frame_offsets"] = frame_offsets
        return res

    def chroma(self, samples, starts, frame_offsets=None, weights=None, norm="max", per_frame=True, summary=False, **params):
        """Host numpy in / numpy out (mgx_chroma_host): the chroma rows of the buffers at `starts` under `weights`
        (a (C, N/2) float32 bank; None: chroma_weights of the plan's size and sample rate with `params`), computed
        on the device from amplitude rows that never cross back. Returns a dict: "chroma" ((F, C) float32) with
        per_frame, "summary" ((S, 4, C) float64: mean, variance, min, max per signal) with summary, which needs
        frame_offsets, and "weights"."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        assert samples.ndim == 1 and starts.ndim == 1
        S = 0
        if frame_offsets is not None:
            frame_offsets = np.ascontiguousarray(frame_offsets, dtype=np.uint64)
            assert frame_offsets.ndim == 1 and frame_offsets.size >= 1
            S = frame_offsets.size - 1
        if weights is None:
            weights = chroma_weights(self.n, self.desc.sample_rate, **params)
        elif params:
            raise TypeError("chroma parameters are given with weights=None")
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        assert weights.ndim == 2 and weights.shape[1] == self.n // 2
        C = weights.shape[0]
        req = ChromaRequest()
        req.struct_size = ctypes.sizeof(ChromaRequest)
        req.num_chroma, req.norm, req.weights = C, _chroma_norm(norm), weights.ctypes.data
        res = {"weights": weights}
        if per_frame:
            res["chroma"] = np.zeros((starts.size, C), np.float32)
            req.per_frame = res["chroma"].ctypes.data
        if summary:
            res["summary"] = np.empty((S, len(STATS), C), np.float64)
            req.summary = res["summary"].ctypes.data
        check(lib().mgx_chroma_host(self._h, samples.ctypes.data, samples.size, starts.ctypes.data, starts.size,
                                    None if frame_offsets is None else frame_offsets.ctypes.data, S, ctypes.byref(req)))
        return res

    def chroma_signals(self, signals, hop, **kw):
        """A list of 1-D host signals in one call (Plan.chroma over signals_frame_starts of their lengths): the
        dict Plan.chroma returns, with "frame_offsets"."""
        signals = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in signals]
        starts, frame_offsets = signals_frame_starts([x.size for x in signals], self.n, hop)
        samples = np.concatenate(signals) if signals else np.empty(0, np.float32)
        res = self.chroma(samples, starts, frame_offsets, **kw)
        res["frame_offsets"] = frame_offsets
        return res

    def hpss(self, samples, starts, frame_offsets=None, kernel_size=None, mode=None, margin=None, power=None, harmonic=False,
             percussive=False, chroma=None, flux=None):
        """Host numpy in / numpy out (mgx_hpss_host): the harmonic / percussive split of the amplitude rows of the
        buffers at `starts` (hpss_params of kernel_size, mode or power, margin), computed on the device from rows that
        never cross back, and what is asked of the two parts. harmonic, percussive: True for the (F, N/2) float32 rows
        ("harmonic", "percussive"; rows of no signal are 0). chroma: a dict of Plan.chroma's options (weights, norm,
        per_frame, summary and the bank's parameters) for the chroma of the harmonic rows: "chroma",
        "chroma_summary", "weights". flux: a dict of mode ("rectified"), lag (1), per_frame (True), summary (False)
        for the flux of the percussive rows: "flux" ((F,) float32), "flux_summary" ((S, 4) float64). A summary needs
        frame_offsets."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        assert samples.ndim == 1 and starts.ndim == 1
        S = 0
        if frame_offsets is not None:
            frame_offsets = np.ascontiguousarray(frame_offsets, dtype=np.uint64)
            assert frame_offsets.ndim == 1 and frame_offsets.size >= 1
            S = frame_offsets.size - 1
        params = hpss_params(kernel_size, mode, margin, power)
        F, cols = starts.size, self.n // 2
        res = {}
        creq = freq = None
        if chroma is not None:
            opts = dict(chroma)
            weights, norm = opts.pop("weights", None), opts.pop("norm", "max")
            per_frame, summary = opts.pop("per_frame", True), opts.pop("summary", False)
            if weights is None:
                weights = chroma_weights(self.n, self.desc.sample_rate, **opts)
            elif opts:
                raise TypeError("chroma parameters are given with weights=None")
            weights = np.ascontiguousarray(weights, dtype=np.float32)
            assert weights.ndim == 2 and weights.shape[1] == cols
            C = weights.shape[0]
            creq = ChromaRequest()
            creq.struct_size = ctypes.sizeof(ChromaRequest)
            creq.num_chroma, creq.norm, creq.weights = C, _chroma_norm(norm), weights.ctypes.data
            res["weights"] = weights
            if per_frame:
                res["chroma"] = np.zeros((F, C), np.float32)
                creq.per_frame = res["chroma"].ctypes.data
            if summary:
                res["chroma_summary"] = np.empty((S, len(STATS), C), np.float64)
                creq.summary = res["chroma_summary"].ctypes.data
        if flux is not None:
            opts = dict(flux)
            fmode, lag = opts.pop("mode", "rectified"), opts.pop("lag", 1)
            per_frame, summary = opts.pop("per_frame", True), opts.pop("summary", False)
            if opts:
                raise TypeError("flux options: mode, lag, per_frame, summary; got %s" % sorted(opts))
            if isinstance(fmode, str):
                if fmode not in FLUX_MODES:
                    raise ValueError("flux mode %r: one of %s" % (fmode, sorted(FLUX_MODES)))
                fmode = FLUX_MODES[fmode]
            freq = FluxRequest()
            freq.struct_size = ctypes.sizeof(FluxRequest)
            freq.field, freq.mode, freq.lag = FLUX_FEATURES["amplitudeSpectrum"], int(fmode), int(lag)
            if per_frame:
                res["flux"] = np.zeros(F, np.float32)
                freq.per_frame = res["flux"].ctypes.data
            if summary:
                res["flux_summary"] = np.empty((S, len(STATS)), np.float64)
                freq.summary = res["flux_summary"].ctypes.data
        if harmonic:
            res["harmonic"] = np.zeros((F, cols), np.float32)
        if percussive:
            res["percussive"] = np.zeros((F, cols), np.float32)
        check(lib().mgx_hpss_host(self._h, samples.ctypes.data, samples.size, starts.ctypes.data, starts.size,
                                  None if frame_offsets is None else frame_offsets.ctypes.data, S, ctypes.byref(params),
                                  None if creq is None else ctypes.byref(creq), None if freq is None else ctypes.byref(freq),
                                  res["harmonic"].ctypes.data if harmonic else None,
                                  res["percussive"].ctypes.data if percussive else None))
        return res

    def hpss_signals(self, signals, hop, **kw):
        """A list of 1-D host signals in one call (Plan.hpss over signals_frame_starts of their lengths): the dict
        Plan.hpss returns, with "frame_offsets"."""
        signals = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in signals]
        starts, frame_offsets = signals_frame_starts([x.size for x in signals], self.n, hop)
        samples = np.concatenate(signals) if signals else np.empty(0, np.float32)
        res = self.hpss(samples, starts, frame_offsets, **kw)
        res["frame_offsets"] = frame_offsets
        return res

    def summarize_signals(self, signals, hop, features, per_frame=(), deltas=None, flux=None):
        """A list of 1-D host signals in one call, pooled per signal: returns (summaries, frame_offsets), summaries
        being {name: ndarray (S, 4, width)} of mean, variance, min, max (STATS) over each signal's buffers; with
        `per_frame`, (summaries, frame_offsets, rows), rows as extract_signals gives them for those features.
        With deltas = (width, order): (summaries, rows, delta_summaries, delta2_summaries) as summarize_gather gives
        them (frame_offsets: signals_frame_starts of the signals' lengths).
        With flux = a list of requests: one more element behind what the call returns without it, the requests' results."""
        signals = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in signals]
        starts, frame_offsets = signals_frame_starts([x.size for x in signals], self.n, hop)
        samples = np.concatenate(signals) if signals else np.empty(0, np.float32)
        if flux is not None:
            r = self.summarize_gather(samples, starts, frame_offsets, features, per_frame, deltas=deltas, flux=flux)
            if deltas is not None:
                return r
            summ, rows, fres = r
            return (summ, frame_offsets, rows, fres) if per_frame else (summ, frame_offsets, fres)
        if deltas is not None:
            return self.summarize_gather(samples, starts, frame_offsets, features, per_frame, deltas=deltas)
        summ, rows = self.summarize_gather(samples, starts, frame_offsets, features, per_frame)
        return (summ, frame_offsets, rows) if per_frame else (summ, frame_offsets)

    def extract_signal(self, samples, hop, features):
        """Host numpy signal in / numpy out, buffers every `hop` samples (stages the signal, not the buffers)."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        assert samples.ndim == 1
        out, o = self._host_outputs(signal_frames(samples.size, self.n, hop), features)
        if _aux(o) is not None:
            check(lib().mgx_extract_host_ex(self._h, samples.ctypes.data, samples.size, hop, ctypes.byref(o), _aux_ref(o)))
            return out
        check(lib().mgx_extract_signal_host(self._h, samples.ctypes.data, samples.size, hop, ctypes.byref(o)))
        return out

    def extract(self, frames, features):
        """Host numpy in / numpy out (stages through the device)."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        F, n = frames.shape
        assert n == self.n
        out, o = self._host_outputs(F, features)
        if _aux(o) is not None:
            check(lib().mgx_extract_host_ex(self._h, frames.ctypes.data, F * n, n, ctypes.byref(o), _aux_ref(o)))
            return out
        check(lib().mgx_extract_host(self._h, frames.ctypes.data, F, ctypes.byref(o)))
        return out

    def extract_pcm(self, pcm, sample_frames, fmt, channels, channel=0, features=(), hop=None):
        """Raw interleaved PCM (bytes / numpy buffer) in host memory -> features of the
        floor(sample_frames / N) buffers of `channel` (decoded on the device); with `hop`, of the
        signal_frames(sample_frames, N, hop) buffers that start every `hop` samples."""
        buf = np.frombuffer(pcm, dtype=np.uint8) if not isinstance(pcm, np.ndarray) else pcm.view(np.uint8)
        buf = np.ascontiguousarray(buf)
        fmt = PCM_FORMATS[fmt] if isinstance(fmt, str) else fmt
        if "melBands" in features:
            h = self.n if hop is None else hop
            out, o = self._host_outputs(signal_frames(sample_frames, self.n, h), features)
            check(lib().mgx_extract_host_pcm_ex(self._h, buf.ctypes.data, buf.size, sample_frames, fmt, channels,
                                                channel, h, ctypes.byref(o), _aux_ref(o)))
            return out
        if hop is None:
            out, o = self._host_outputs(sample_frames // self.n, features)
            check(lib().mgx_extract_host_pcm(self._h, buf.ctypes.data, buf.size, sample_frames, fmt, channels, channel,
                                             ctypes.byref(o)))
            return out
        out, o = self._host_outputs(signal_frames(sample_frames, self.n, hop), features)
        check(lib().mgx_extract_signal_host_pcm(self._h, buf.ctypes.data, buf.size, sample_frames, fmt, channels,
                                                channel, hop, ctypes.byref(o)))
        return out

    def extract_wav(self, wav_bytes, features, channel=0, hop=None):
        """A whole .wav file (bytes) -> features of its full buffers (channel `channel`), disjoint or,
        with `hop`, every `hop` samples."""
        info = wav_parse(wav_bytes)
        data = np.frombuffer(wav_bytes, dtype=np.uint8)[info["data_offset"]:info["data_offset"] + info["data_bytes"]]
        return self.extract_pcm(data, info["sample_frames"], info["pcm_format"], info["channels"], channel, features,
                                hop=hop)

    def _host_outputs(self, F, features):
        n = self.n
        L = n // 2
        out, o = {}, Outputs()
        sd = self.scalar_dtype
        for f in features:
            if f in SCALAR_NAMES:
                out[f] = np.empty(F, sd)
                o.scalars[SCALAR_NAMES.index(f)] = out[f].ctypes.data
            elif f == "loudness":
                out["loudness.specific"] = np.empty((F, NUM_BARK), np.float32)
                out["loudness.total"] = np.empty(F, sd)
                o.loudness_specific = out["loudness.specific"].ctypes.data
                o.scalars[10] = out["loudness.total"].ctypes.data
            elif f == "mfcc":
                out[f] = np.empty((F, self.desc.num_mfcc_coeffs), np.float32)
                o.mfcc = out[f].ctypes.data
            elif f == "melBands":
                out[f] = np.empty((F, self.desc.num_mel_bands), np.float32)
                _set_mel_bands(o, out[f].ctypes.data)
            elif f == "amplitudeSpectrum":
                out[f] = np.empty((F, L), np.float32)
                o.amplitude_spectrum = out[f].ctypes.data
            elif f == "powerSpectrum":
                out[f] = np.empty((F, L), np.float32)
                o.power_spectrum = out[f].ctypes.data
            elif f == "complexSpectrum":
                out["complexSpectrum.real"] = np.empty((F, n), np.float32)
                out["complexSpectrum.imag"] = np.empty((F, n), np.float32)
                o.complex_real = out["complexSpectrum.real"].ctypes.data
                o.complex_imag = out["complexSpectrum.imag"].ctypes.data
            else:
                raise ValueError("unknown feature %r" % f)
        return out, o


ALL_FEATURES = SCALAR_NAMES[:10] + ["loudness", "perceptualSpread", "perceptualSharpness", "mfcc"]


def shard_range(total, nranks, rank):
    """(start, count) of rank's contiguous shard (mgx_shard_range; host only)."""
    s, c = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib().mgx_shard_range(total, nranks, rank, ctypes.byref(s), ctypes.byref(c)))
    return s.value, c.value


def output_mask(outputs):
    """MGX_OUT_* mask of the non-NULL fields of an Outputs structure."""
    m = 0
    for i in range(NUM_SCALARS):
        if outputs.scalars[i]:
            m |= 1 << i
    for bit, f in ((13, "loudness_specific"), (14, "mfcc"), (15, "amplitude_spectrum"),
                   (16, "power_spectrum"), (17, "complex_real")):
        if getattr(outputs, f):
            m |= 1 << bit
    return m


def packed_layout(desc, mask, num_frames):
    """(total_bytes, {field: offset}) of mgx_packed_layout (host only)."""
    off = (ctypes.c_uint64 * 19)()
    total = lib().mgx_packed_layout(ctypes.byref(desc), mask, num_frames, off)
    return total, {FIELDS[i]: off[i] for i in range(19) if off[i] != 2 ** 64 - 1}


def comm_unique_id():
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    check(lib().mgx_comm_unique_id(buf, COMM_ID_BYTES))
    return buf.raw


class Group:
    """Frames sharded over several devices with an RCCL gather of the feature records to the
    root (rank 0) — include/meyda_gpu.h "Multi-device groups".

    Group(devices=[0, 1, ...], **plan_kw)                 one process, several devices
    Group(rank=r, nranks=n, unique_id=b, device=d, ...)   one process per device (torchrun)
    Group(loopback=n, device=d, ...)                      test transport: n ranks on one device,
                                                          chunks as device copies
    Group(loopback=n, transport="rccl", device=d, ...)    the same, chunks as RCCL send/recv to
                                                          self on a one-rank communicator
    """

    def __init__(self, buffer_size=512, devices=None, rank=None, nranks=None, unique_id=None, loopback=None,
                 transport="copy", **kw):
        h = ctypes.c_void_p()
        if loopback is not None:
            self.desc = make_desc(buffer_size=buffer_size, **kw)
            create = {"copy": lib().mgx_group_create_loopback, "rccl": lib().mgx_group_create_loopback_rccl}[transport]
            check(create(ctypes.byref(self.desc), loopback, ctypes.byref(h)))
        elif devices is not None:
            self.desc = make_desc(buffer_size=buffer_size, device=devices[0], **kw)
            arr = (ctypes.c_int32 * len(devices))(*devices)
            check(lib().mgx_group_create(ctypes.byref(self.desc), arr, len(devices), ctypes.byref(h)))
        else:
            self.desc = make_desc(buffer_size=buffer_size, **kw)
            check(lib().mgx_group_create_rank(ctypes.byref(self.desc), unique_id, nranks, rank, ctypes.byref(h)))
        self._h = h
        self.n = buffer_size
        self.scalar_dtype = np.float64 if kw.get("scalar_f64") else np.float32
        nr, first, nl = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().mgx_group_info(h, ctypes.byref(nr), ctypes.byref(first), ctypes.byref(nl)))
        self.nranks, self.first_local, self.num_local = nr.value, first.value, nl.value

    def comm_info(self):
        """(ranks, rank, device) as this process's RCCL communicator reports them, or
        (-1, -1, -1) without one (mgx_group_comm_info)."""
        n, r, d = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(lib().mgx_group_comm_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(d)))
        return n.value, r.value, d.value

    def close(self):
        if getattr(self, "_h", None):
            lib().mgx_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def extract_device(self, frames_ptrs, counts, root_outputs, mask, num_chunks=0, streams=None):
        """frames_ptrs: device pointers of the local ranks' shards; counts: frames of every
        rank; root_outputs: an Outputs of device pointers on the root (None elsewhere)."""
        fp = (ctypes.c_void_p * len(frames_ptrs))(*frames_ptrs)
        cn = (ctypes.c_uint64 * len(counts))(*counts)
        st = None if streams is None else (ctypes.c_void_p * len(streams))(*streams)
        check(lib().mgx_group_extract_device(self._h, fp, cn, None if root_outputs is None else ctypes.byref(root_outputs),
                                             mask, num_chunks, st))

    def extract(self, frames, features):
        """Host numpy in / numpy out, sharded over the group's devices (single process)."""
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        F, n = frames.shape
        assert n == self.n
        if "melBands" in features:
            raise ValueError("multi-device groups take no auxiliary outputs (melBands): include/meyda_gpu.h")
        out, o = Plan._host_outputs(self, F, features)
        check(lib().mgx_group_extract_host(self._h, frames.ctypes.data, F, ctypes.byref(o)))
        return out


def synth_frames_device(tensor, seed, first_frame=0, stream=None):
    """Fill a (F, N) float32 CUDA tensor with the synthetic PCM of SURVEY.md §8(d)."""
    import torch
    F, n = tensor.shape
    if stream is None:
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
    check(lib().mgx_synth_frames_device(ctypes.c_void_p(tensor.data_ptr()), F, n, seed, first_frame,
                                        ctypes.c_void_p(stream)))


def wav_parse(data):
    """RIFF/WAVE header of `data` (bytes): format, channels, rate, data offset/size (no GPU)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    info = WavInfo()
    info.struct_size = ctypes.sizeof(WavInfo)
    check(lib().mgx_wav_parse(buf.ctypes.data, buf.size, ctypes.byref(info)))
    return {k: getattr(info, k) for k, _ in WavInfo._fields_ if k != "struct_size"}


def pcm_decode_device(pcm_u8, sample_frames, fmt, channels, channel, out, stream=None):
    """Decode interleaved PCM (a uint8 CUDA tensor) into `out` (float32 CUDA tensor)."""
    import torch
    fmt = PCM_FORMATS[fmt] if isinstance(fmt, str) else fmt
    if stream is None:
        stream = torch.cuda.current_stream(out.device).cuda_stream
    check(lib().mgx_pcm_decode_device(ctypes.c_void_p(pcm_u8.data_ptr()), sample_frames, fmt, channels, channel,
                                      ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)))


def delta_device(rows_ptr, num_frames, cols, rows_f64, offsets_ptr, num_signals, width, delta_ptr, delta2_ptr, stream=None):
    """mgx_delta_device on device pointers (async on `stream`); a pointer may be None."""
    check(lib().mgx_delta_device(ctypes.c_void_p(rows_ptr or 0), num_frames, cols, 1 if rows_f64 else 0,
                                 ctypes.c_void_p(offsets_ptr or 0), num_signals, width, ctypes.c_void_p(delta_ptr or 0),
                                 ctypes.c_void_p(delta2_ptr or 0), ctypes.c_void_p(stream or 0)))


def delta_torch(rows, frame_offsets=None, width=2, order=2, stream=None):
    """The regression deltas of `rows`, a (F,) or (F, cols) float32 or float64 CUDA tensor, within each signal:
    signal s owns rows [frame_offsets[s], frame_offsets[s + 1]) (an int64 CUDA tensor, or anything numpy turns
    into one; None: one signal, every row). Returns the tuple of tensors of rows' shape, (delta,) at order 1 and
    (delta, delta2) at order 2; rows that belong to no signal are 0."""
    import torch
    assert rows.is_cuda and rows.is_contiguous() and rows.dim() in (1, 2) and rows.dtype in (torch.float32, torch.float64)
    if order not in (1, 2):
        raise ValueError("delta order %r: 1 or 2" % (order,))
    F = rows.shape[0]
    cols = rows.shape[1] if rows.dim() == 2 else 1
    S = 0
    if frame_offsets is not None:
        if not torch.is_tensor(frame_offsets):
            frame_offsets = torch.from_numpy(np.ascontiguousarray(frame_offsets, dtype=np.uint64).view(np.int64)).to(rows.device)
        assert frame_offsets.is_cuda and frame_offsets.dtype == torch.int64 and frame_offsets.is_contiguous()
        assert frame_offsets.dim() == 1 and frame_offsets.shape[0] >= 1
        S = frame_offsets.shape[0] - 1
    out = tuple(torch.zeros_like(rows) for _ in range(order))
    if stream is None:
        stream = torch.cuda.current_stream(rows.device).cuda_stream
    delta_device(rows.data_ptr(), F, cols, rows.dtype == torch.float64, None if frame_offsets is None else frame_offsets.data_ptr(),
                 S, width, out[0].data_ptr(), out[1].data_ptr() if order == 2 else None, stream)
    return out


def flux_device(rows_ptr, num_frames, cols, rows_f64, offsets_ptr, num_signals, mode, lag, flux_ptr, stream=None):
    """mgx_flux_device on device pointers (async on `stream`); a pointer may be None."""
    check(lib().mgx_flux_device(ctypes.c_void_p(rows_ptr or 0), num_frames, cols, 1 if rows_f64 else 0,
                                ctypes.c_void_p(offsets_ptr or 0), num_signals, mode, lag, ctypes.c_void_p(flux_ptr or 0),
                                ctypes.c_void_p(stream or 0)))


def flux_torch(rows, frame_offsets=None, mode="rectified", lag=1, stream=None, out=None):
    """The spectral flux of `rows`, a (F,) or (F, cols) float32 or float64 CUDA tensor, within each signal: the
    distance of every row from the row `lag` before it, clamped at the signal's first row (include/meyda_gpu.h).
    mode: "rectified", "l1" or "l2". Signal s owns rows [frame_offsets[s], frame_offsets[s + 1]) (an int64 CUDA
    tensor, or anything numpy turns into one; None: one signal, every row). Returns a (F,) tensor of rows' type
    (`out` when given, written where a row belongs to a signal); rows that belong to no signal are 0."""
    import torch
    assert rows.is_cuda and rows.is_contiguous() and rows.dim() in (1, 2) and rows.dtype in (torch.float32, torch.float64)
    if isinstance(mode, str):
        if mode not in FLUX_MODES:
            raise ValueError("flux mode %r: one of %s" % (mode, sorted(FLUX_MODES)))
        mode = FLUX_MODES[mode]
    F = rows.shape[0]
    cols = rows.shape[1] if rows.dim() == 2 else 1
    S = 0
    if frame_offsets is not None:
        if not torch.is_tensor(frame_offsets):
            frame_offsets = torch.from_numpy(np.ascontiguousarray(frame_offsets, dtype=np.uint64).view(np.int64)).to(rows.device)
        assert frame_offsets.is_cuda and frame_offsets.dtype == torch.int64 and frame_offsets.is_contiguous()
        assert frame_offsets.dim() == 1 and frame_offsets.shape[0] >= 1
        S = frame_offsets.shape[0] - 1
    if out is None:
        out = torch.zeros(F, dtype=rows.dtype, device=rows.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == rows.dtype and out.shape == (F,)
    if stream is None:
        stream = torch.cuda.current_stream(rows.device).cuda_stream
    flux_device(rows.data_ptr(), F, cols, rows.dtype == torch.float64, None if frame_offsets is None else frame_offsets.data_ptr(),
                S, mode, lag, out.data_ptr(), stream)
    return out


def peaks_workspace_bytes(num_frames, num_signals=0):
    """mgx_peaks_workspace_bytes (host only)."""
    b = ctypes.c_uint64()
    check(lib().mgx_peaks_workspace_bytes(num_frames, num_signals, ctypes.byref(b)))
    return b.value


def peaks_device(envelope_ptr, num_frames, envelope_f64, offsets_ptr, num_signals, params, out, workspace_ptr, workspace_bytes,
                 stream=None):
    """mgx_peaks_device on device pointers (async on `stream`); params: a PeakParams, out: a PeakOutputs; a pointer may be None."""
    check(lib().mgx_peaks_device(ctypes.c_void_p(envelope_ptr or 0), num_frames, 1 if envelope_f64 else 0,
                                 ctypes.c_void_p(offsets_ptr or 0), num_signals, ctypes.byref(params), ctypes.byref(out),
                                 ctypes.c_void_p(workspace_ptr or 0), workspace_bytes, ctypes.c_void_p(stream or 0)))


def peaks_torch(envelope, frame_offsets=None, capacity=None, starts=None, stream=None, mask_fill=0, **params):
    """The peaks of `envelope`, a (F,) float32 or float64 CUDA tensor, within each signal (include/meyda_gpu.h):
    params are pre_max, post_max, pre_avg, post_avg, delta, wait. Signal s owns rows [frame_offsets[s],
    frame_offsets[s + 1]) (an int64 CUDA tensor, or anything numpy turns into one; None: one signal, every row).
    Returns (mask, peak_offsets, peaks) -- a (F,) uint8 tensor, `mask_fill` in rows that belong to no signal; a
    (S + 1,) int64 tensor of the true counts; a (capacity,) int64 tensor of row indices, of which the first
    min(peak_offsets[S], capacity) are written (capacity None: F, which always holds them) -- and, with `starts`
    (the gather table the rows came from), a fourth tensor: starts[peaks[i]], the next launch's table.
    The workspace is allocated here, as summarize_gather_torch allocates its own."""
    import torch
    assert envelope.is_cuda and envelope.is_contiguous() and envelope.dim() == 1
    assert envelope.dtype in (torch.float32, torch.float64)
    dev = envelope.device
    F = envelope.shape[0]
    S = 0
    if frame_offsets is not None:
        if not torch.is_tensor(frame_offsets):
            frame_offsets = torch.from_numpy(np.ascontiguousarray(frame_offsets, dtype=np.uint64).view(np.int64)).to(dev)
        assert frame_offsets.is_cuda and frame_offsets.dtype == torch.int64 and frame_offsets.is_contiguous()
        assert frame_offsets.dim() == 1 and frame_offsets.shape[0] >= 1
        S = frame_offsets.shape[0] - 1
    if capacity is None:
        capacity = max(F, 1)
    mask = torch.full((F,), mask_fill, dtype=torch.uint8, device=dev)
    offsets = torch.zeros((S if frame_offsets is not None else 1) + 1, dtype=torch.int64, device=dev)
    peaks = torch.zeros(capacity, dtype=torch.int64, device=dev)
    o = PeakOutputs()
    o.struct_size = ctypes.sizeof(PeakOutputs)
    o.mask, o.peak_offsets, o.peaks, o.capacity = mask.data_ptr(), offsets.data_ptr(), peaks.data_ptr(), capacity
    peak_starts = None
    if starts is not None:
        if not torch.is_tensor(starts):
            starts = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint64).view(np.int64)).to(dev)
        assert starts.is_cuda and starts.dtype == torch.int64 and starts.is_contiguous() and starts.shape == (F,)
        peak_starts = torch.zeros(capacity, dtype=torch.int64, device=dev)
        o.starts, o.peak_starts = starts.data_ptr(), peak_starts.data_ptr()
    nbytes = peaks_workspace_bytes(F, S)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    peaks_device(envelope.data_ptr(), F, envelope.dtype == torch.float64, None if frame_offsets is None else frame_offsets.data_ptr(),
                 S, peak_params(**params), o, ws.data_ptr(), nbytes, stream)
    return (mask, offsets, peaks) if starts is None else (mask, offsets, peaks, peak_starts)


def chroma_weights(n, sample_rate, **params):
    """mgx_chroma_weights (host only): the (C, n/2) float32 chroma filter bank of librosa.filters.chroma for buffers
    of n samples; params: num_chroma (12), a440 (440), center_octave (5), octave_width (2; 0: none), base_c (True)."""
    p = chroma_params(**params)
    w = np.zeros((max(int(p.num_chroma), 0), max(int(n) // 2, 0)), np.float32)
    # (a refused size or C may leave nothing to point at: the library checks them before it writes)
    buf = w if w.size else np.zeros(1, np.float32)
    check(lib().mgx_chroma_weights(int(n), float(sample_rate), ctypes.byref(p), buf.ctypes.data))
    return w


def chroma_device(rows_ptr, num_frames, cols, weights_ptr, num_chroma, norm, chroma_ptr, stream=None):
    """mgx_chroma_device on device pointers (async on `stream`); a pointer may be None."""
    check(lib().mgx_chroma_device(ctypes.c_void_p(rows_ptr or 0), num_frames, cols, ctypes.c_void_p(weights_ptr or 0),
                                  num_chroma, norm, ctypes.c_void_p(chroma_ptr or 0), ctypes.c_void_p(stream or 0)))


def chroma_torch(rows, weights, norm="max", stream=None, out=None):
    """The chroma rows of `rows`, a (F, cols) float32 CUDA tensor, under `weights`, a (C, cols) float32 CUDA tensor
    (or anything numpy turns into one): the products added in the fixed order of include/meyda_gpu.h, then divided
    by the row's maximum (norm "max") or left as they are ("none"). Returns a (F, C) float32 tensor (`out` when given)."""
    import torch
    assert rows.is_cuda and rows.is_contiguous() and rows.dim() == 2 and rows.dtype == torch.float32
    if not torch.is_tensor(weights):
        weights = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32)).to(rows.device)
    assert weights.is_cuda and weights.is_contiguous() and weights.dim() == 2 and weights.dtype == torch.float32
    F, cols = rows.shape
    C = weights.shape[0]
    assert weights.shape[1] == cols
    if out is None:
        out = torch.zeros((F, C), dtype=torch.float32, device=rows.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.shape == (F, C)
    if stream is None:
        stream = torch.cuda.current_stream(rows.device).cuda_stream
    chroma_device(rows.data_ptr(), F, cols, weights.data_ptr(), C, _chroma_norm(norm), out.data_ptr(), stream)
    return out


def hpss_device(rows_ptr, num_frames, cols, offsets_ptr, num_signals, params, harmonic_ptr, percussive_ptr, stream=None):
    """mgx_hpss_device on device pointers (async on `stream`); a pointer may be None. params: an HpssParams."""
    check(lib().mgx_hpss_device(ctypes.c_void_p(rows_ptr or 0), num_frames, cols, ctypes.c_void_p(offsets_ptr or 0), num_signals,
                                None if params is None else ctypes.byref(params), ctypes.c_void_p(harmonic_ptr or 0),
                                ctypes.c_void_p(percussive_ptr or 0), ctypes.c_void_p(stream or 0)))


def hpss_torch(rows, frame_offsets=None, kernel_size=None, mode=None, margin=None, power=None, harmonic=True, percussive=True,
               stream=None, out_harmonic=None, out_percussive=None):
    """The harmonic / percussive split of `rows`, a (F, cols) float32 CUDA tensor, within each signal: the median
    along time and the median along frequency under the IEEE total order, with reflected ends, and the masks of
    include/meyda_gpu.h (hpss_params of kernel_size, mode or power, margin; mode "medians": the two medians). Signal
    s owns rows [frame_offsets[s], frame_offsets[s + 1]) (an int64 CUDA tensor, or anything numpy turns into one;
    None: one signal, every row). Returns (harmonic, percussive), (F, cols) float32 tensors (the `out_` ones when
    given, written where a row belongs to a signal; else rows of no signal are 0), None for a part not asked for."""
    import torch
    assert rows.is_cuda and rows.is_contiguous() and rows.dim() == 2 and rows.dtype == torch.float32
    params = hpss_params(kernel_size, mode, margin, power)
    F, cols = rows.shape
    S = 0
    if frame_offsets is not None:
        if not torch.is_tensor(frame_offsets):
            frame_offsets = torch.from_numpy(np.ascontiguousarray(frame_offsets, dtype=np.uint64).view(np.int64)).to(rows.device)
        assert frame_offsets.is_cuda and frame_offsets.dtype == torch.int64 and frame_offsets.is_contiguous()
        assert frame_offsets.dim() == 1 and frame_offsets.shape[0] >= 1
        S = frame_offsets.shape[0] - 1
    outs = []
    for want, out in ((harmonic, out_harmonic), (percussive, out_percussive)):
        if out is None and want:
            out = torch.zeros((F, cols), dtype=torch.float32, device=rows.device)
        if out is not None:
            assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.shape == (F, cols)
        outs.append(out)
    if stream is None:
        stream = torch.cuda.current_stream(rows.device).cuda_stream
    hpss_device(rows.data_ptr(), F, cols, None if frame_offsets is None else frame_offsets.data_ptr(), S, params,
                None if outs[0] is None else outs[0].data_ptr(), None if outs[1] is None else outs[1].data_ptr(), stream)
    return outs[0], outs[1]


def tempogram_window(win_length):
    """mgx_tempogram_window (host only): the periodic Hann window of win_length float32 values."""
    h = np.zeros(max(int(win_length), 0), np.float32)
    buf = h if h.size else np.zeros(1, np.float32)
    check(lib().mgx_tempogram_window(int(win_length), buf.ctypes.data))
    return h


def tempo_prior(frame_rate, num_lags, start_bpm=120.0, std_octaves=1.0, max_bpm=320.0):
    """mgx_tempo_prior (host only): librosa's log-normal tempo prior over the lags 0 .. num_lags - 1 of an envelope of
    frame_rate rows per second, without its constant factor; p[0] = 0, and 0 above max_bpm (0: no limit)."""
    p = np.zeros(max(int(num_lags), 0), np.float64)
    buf = p if p.size else np.zeros(1, np.float64)
    check(lib().mgx_tempo_prior(float(frame_rate), float(start_bpm), float(std_octaves), float(max_bpm), int(num_lags),
                                buf.ctypes.data))
    return p


def lag_bpm(lag, frame_rate):
    """60 frame_rate / lag as float64, NaN where the lag is 0 (no tempo)."""
    lag = np.asarray(lag, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(lag > 0, 60.0 * float(frame_rate) / np.where(lag > 0, lag, 1.0), np.nan)


def tempogram_device(envelope_ptr, num_frames, envelope_f64, offsets_ptr, num_signals, window_ptr, win_length, num_lags, norm,
                     tempogram_ptr, stream=None):
    """mgx_tempogram_device on device pointers (async on `stream`); a pointer may be None."""
    check(lib().mgx_tempogram_device(ctypes.c_void_p(envelope_ptr or 0), num_frames, 1 if envelope_f64 else 0,
                                     ctypes.c_void_p(offsets_ptr or 0), num_signals, ctypes.c_void_p(window_ptr or 0), win_length,
                                     num_lags, norm, ctypes.c_void_p(tempogram_ptr or 0), ctypes.c_void_p(stream or 0)))


def tempo_workspace_bytes(num_frames, num_signals, params, keep_rows):
    """mgx_tempo_workspace_bytes (host only); params: a TempoParams; keep_rows: the call has a tempogram output."""
    b = ctypes.c_uint64()
    check(lib().mgx_tempo_workspace_bytes(num_frames, num_signals, ctypes.byref(params), 1 if keep_rows else 0, ctypes.byref(b)))
    return b.value


def tempo_device(envelope_ptr, num_frames, envelope_f64, offsets_ptr, num_signals, params, window_ptr, prior_ptr, tempogram_ptr,
                 summary_ptr, lag_ptr, workspace_ptr, workspace_bytes, stream=None):
    """mgx_tempo_device on device pointers (async on `stream`); params: a TempoParams; a pointer may be None."""
    check(lib().mgx_tempo_device(ctypes.c_void_p(envelope_ptr or 0), num_frames, 1 if envelope_f64 else 0,
                                 ctypes.c_void_p(offsets_ptr or 0), num_signals, ctypes.byref(params),
                                 ctypes.c_void_p(window_ptr or 0), ctypes.c_void_p(prior_ptr or 0), ctypes.c_void_p(tempogram_ptr or 0),
                                 ctypes.c_void_p(summary_ptr or 0), ctypes.c_void_p(lag_ptr or 0), ctypes.c_void_p(workspace_ptr or 0),
                                 workspace_bytes, ctypes.c_void_p(stream or 0)))


def _device_table(frame_offsets, dev):
    import torch
    if frame_offsets is None:
        return None, 0
    if not torch.is_tensor(frame_offsets):
        frame_offsets = torch.from_numpy(np.ascontiguousarray(frame_offsets, dtype=np.uint64).view(np.int64)).to(dev)
    assert frame_offsets.is_cuda and frame_offsets.dtype == torch.int64 and frame_offsets.is_contiguous()
    assert frame_offsets.dim() == 1 and frame_offsets.shape[0] >= 1
    return frame_offsets, frame_offsets.shape[0] - 1


def tempogram_torch(envelope, window, frame_offsets=None, num_lags=None, norm="lag0", stream=None, out=None):
    """The autocorrelation tempogram of `envelope`, a (F,) float32 or float64 CUDA tensor, under `window`, a (W,)
    float32 CUDA tensor, within each signal (include/meyda_gpu.h): a (F, L) float32 tensor, L = num_lags (None: W).
    Signal s owns rows [frame_offsets[s], frame_offsets[s + 1]) (an int64 CUDA tensor, or anything numpy turns into
    one; None: one signal, every row); rows of no signal keep what `out` held (zero when it is allocated here)."""
    import torch
    assert envelope.is_cuda and envelope.is_contiguous() and envelope.dim() == 1
    assert envelope.dtype in (torch.float32, torch.float64)
    assert window.is_cuda and window.is_contiguous() and window.dim() == 1 and window.dtype == torch.float32
    dev = envelope.device
    F, W = envelope.shape[0], window.shape[0]
    L = W if num_lags is None else int(num_lags)
    frame_offsets, S = _device_table(frame_offsets, dev)
    if out is None:
        out = torch.zeros((F, max(L, 0)), dtype=torch.float32, device=dev)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.shape == (F, L)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    tempogram_device(envelope.data_ptr(), F, envelope.dtype == torch.float64, None if frame_offsets is None else frame_offsets.data_ptr(),
                     S, window.data_ptr(), W, L, _tempogram_norm(norm), out.data_ptr(), stream)
    return out


def tempo_torch(envelope, window, prior=None, frame_offsets=None, num_lags=None, norm="lag0", gain=1e6, tempogram=False,
                summary=True, stream=None, workspace=None):
    """mgx_tempo_device on CUDA tensors: the tempogram of `envelope` under `window` (as tempogram_torch), pooled per
    signal, and the lag `prior` (a (L,) float64 CUDA tensor; None: no pick) picks from the mean row. Returns a dict
    with "lag" ((S,) int32, with a prior), "summary" ((S, 4, L) float64, with summary) and "tempogram" ((F, L)
    float32, zero in rows of no signal, with tempogram=True or a tensor to write into). Without a tempogram the
    rows pass through the workspace TEMPO_CHUNK_ROWS at a time. The workspace is allocated here unless one is given
    (a uint8 CUDA tensor of tempo_workspace_bytes, for a capture)."""
    import torch
    assert envelope.is_cuda and envelope.is_contiguous() and envelope.dim() == 1
    assert envelope.dtype in (torch.float32, torch.float64)
    assert window.is_cuda and window.is_contiguous() and window.dim() == 1 and window.dtype == torch.float32
    dev = envelope.device
    F, W = envelope.shape[0], window.shape[0]
    tp = tempo_params(W, num_lags, norm, gain)
    L = int(tp.num_lags)
    frame_offsets, S = _device_table(frame_offsets, dev)
    Sout = S if frame_offsets is not None else 1
    res = {}
    if tempogram is True:
        tempogram = torch.zeros((F, L), dtype=torch.float32, device=dev)
    if tempogram is not None and tempogram is not False:
        assert tempogram.is_cuda and tempogram.is_contiguous() and tempogram.dtype == torch.float32 and tempogram.shape == (F, L)
        res["tempogram"] = tempogram
    else:
        tempogram = None
    if summary:
        res["summary"] = torch.empty((Sout, len(STATS), L), dtype=torch.float64, device=dev)
    if prior is not None:
        assert prior.is_cuda and prior.is_contiguous() and prior.dtype == torch.float64 and prior.shape == (L,)
        res["lag"] = torch.zeros(Sout, dtype=torch.int32, device=dev)
    nbytes = tempo_workspace_bytes(F, S, tp, tempogram is not None)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    assert workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.numel() >= nbytes
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    tempo_device(envelope.data_ptr(), F, envelope.dtype == torch.float64, None if frame_offsets is None else frame_offsets.data_ptr(),
                 S, tp, window.data_ptr(), None if prior is None else prior.data_ptr(), None if tempogram is None else tempogram.data_ptr(),
                 res["summary"].data_ptr() if summary else None, res["lag"].data_ptr() if prior is not None else None,
                 workspace.data_ptr(), workspace.numel(), stream)
    return res


def beat_tables(max_period, tightness=100.0):
    """mgx_beat_tables (host only): (gauss, penalty) -- (P + 1)(P + 2) / 2 float32 and (P + 1)^2 float64 -- for the
    periods 1 .. max_period (include/meyda_gpu.h)."""
    P = int(max_period)
    ok = 1 <= P <= BEAT_MAX_PERIOD
    # (a refused size leaves nothing to size the arrays by: the library checks it before it writes)
    gauss = np.zeros((P + 1) * (P + 2) // 2 if ok else 1, np.float32)
    penalty = np.zeros((P + 1) ** 2 if ok else 1, np.float64)
    check(lib().mgx_beat_tables(P if 0 <= P < 2 ** 32 else 0, float(tightness), gauss.ctypes.data, penalty.ctypes.data))
    return gauss, penalty


def beats_workspace_bytes(num_frames, num_signals=0):
    """mgx_beats_workspace_bytes (host only)."""
    b = ctypes.c_uint64()
    check(lib().mgx_beats_workspace_bytes(num_frames, num_signals, ctypes.byref(b)))
    return b.value


def beats_device(envelope_ptr, num_frames, envelope_f64, offsets_ptr, num_signals, period_ptr, params, gauss_ptr, penalty_ptr,
                 local_score_ptr, cum_score_ptr, out, workspace_ptr, workspace_bytes, stream=None):
    """mgx_beats_device on device pointers (async on `stream`); params: a BeatParams, out: a PeakOutputs; a pointer may be None."""
    check(lib().mgx_beats_device(ctypes.c_void_p(envelope_ptr or 0), num_frames, 1 if envelope_f64 else 0,
                                 ctypes.c_void_p(offsets_ptr or 0), num_signals, ctypes.c_void_p(period_ptr or 0), ctypes.byref(params),
                                 ctypes.c_void_p(gauss_ptr or 0), ctypes.c_void_p(penalty_ptr or 0), ctypes.c_void_p(local_score_ptr or 0),
                                 ctypes.c_void_p(cum_score_ptr or 0), ctypes.byref(out), ctypes.c_void_p(workspace_ptr or 0),
                                 workspace_bytes, ctypes.c_void_p(stream or 0)))


def beats_torch(envelope, period, gauss, penalty, frame_offsets=None, max_period=None, trim=True, capacity=None, starts=None,
                scores=False, stream=None, workspace=None, mask_fill=0, score_fill=0.0):
    """mgx_beats_device on CUDA tensors: the beats of `envelope`, a (F,) float32 or float64 tensor, within each signal
    (frame_offsets as peaks_torch takes them) at the signal's entry of `period`, an (S,) int32 tensor -- the "lag" of
    tempo_torch as it is -- under the tables of beat_tables(max_period) (tensors, or anything numpy turns into them;
    max_period None: from the size of penalty). Returns a dict: "mask" ((F,) uint8, `mask_fill` in rows of no
    signal), "peak_offsets" ((S + 1,) int64: the true counts), "peaks" ((capacity,) int64, the first
    min(peak_offsets[S], capacity) written; capacity None: F), with `starts` "peak_starts", and with scores=True
    "local_score" and "cum_score" ((F,) float64, `score_fill` in rows of no signal). workspace: a uint8 CUDA tensor
    of beats_workspace_bytes (for a capture), None: allocated here."""
    import torch
    assert envelope.is_cuda and envelope.is_contiguous() and envelope.dim() == 1
    assert envelope.dtype in (torch.float32, torch.float64)
    dev = envelope.device
    F = envelope.shape[0]
    S = 0
    if frame_offsets is not None:
        if not torch.is_tensor(frame_offsets):
            frame_offsets = torch.from_numpy(np.ascontiguousarray(frame_offsets, dtype=np.uint64).view(np.int64)).to(dev)
        assert frame_offsets.is_cuda and frame_offsets.dtype == torch.int64 and frame_offsets.is_contiguous()
        assert frame_offsets.dim() == 1 and frame_offsets.shape[0] >= 1
        S = frame_offsets.shape[0] - 1
    nsig = S if frame_offsets is not None else 1
    if not torch.is_tensor(period):
        period = torch.from_numpy(np.ascontiguousarray(period, dtype=np.uint32).view(np.int32)).to(dev)
    assert period.is_cuda and period.is_contiguous() and period.dtype == torch.int32 and period.shape == (nsig,)
    if not torch.is_tensor(gauss):
        gauss = torch.from_numpy(np.ascontiguousarray(gauss, dtype=np.float32)).to(dev)
    if not torch.is_tensor(penalty):
        penalty = torch.from_numpy(np.ascontiguousarray(penalty, dtype=np.float64)).to(dev)
    assert gauss.is_cuda and gauss.is_contiguous() and gauss.dtype == torch.float32 and gauss.dim() == 1
    assert penalty.is_cuda and penalty.is_contiguous() and penalty.dtype == torch.float64 and penalty.dim() == 1
    if max_period is None:
        max_period = int(round(penalty.shape[0] ** 0.5)) - 1
    bp = beat_params(max_period, trim)
    P = int(bp.max_period)
    if 1 <= P <= BEAT_MAX_PERIOD:
        assert gauss.shape[0] == (P + 1) * (P + 2) // 2 and penalty.shape[0] == (P + 1) ** 2
    if capacity is None:
        capacity = max(F, 1)
    res = {"mask": torch.full((F,), mask_fill, dtype=torch.uint8, device=dev),
           "peak_offsets": torch.zeros(nsig + 1, dtype=torch.int64, device=dev),
           "peaks": torch.zeros(capacity, dtype=torch.int64, device=dev)}
    o = PeakOutputs()
    o.struct_size = ctypes.sizeof(PeakOutputs)
    o.mask, o.peak_offsets, o.peaks, o.capacity = res["mask"].data_ptr(), res["peak_offsets"].data_ptr(), res["peaks"].data_ptr(), capacity
    if starts is not None:
        if not torch.is_tensor(starts):
            starts = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.uint64).view(np.int64)).to(dev)
        assert starts.is_cuda and starts.dtype == torch.int64 and starts.is_contiguous() and starts.shape == (F,)
        res["peak_starts"] = torch.zeros(capacity, dtype=torch.int64, device=dev)
        o.starts, o.peak_starts = starts.data_ptr(), res["peak_starts"].data_ptr()
    if scores:
        res["local_score"] = torch.full((F,), score_fill, dtype=torch.float64, device=dev)
        res["cum_score"] = torch.full((F,), score_fill, dtype=torch.float64, device=dev)
    nbytes = beats_workspace_bytes(F, S)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    assert workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.numel() >= nbytes
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    beats_device(envelope.data_ptr(), F, envelope.dtype == torch.float64, None if frame_offsets is None else frame_offsets.data_ptr(),
                 S, period.data_ptr(), bp, gauss.data_ptr(), penalty.data_ptr(),
                 res["local_score"].data_ptr() if scores else None, res["cum_score"].data_ptr() if scores else None, o,
                 workspace.data_ptr(), nbytes, stream)
    return res
