"""mgx_signal_frames (no GPU needed): the number of buffers of N samples that start every `hop` samples in
a signal of S samples, F = (S < N) ? 0 : (S - N) / hop + 1 -- the one definition every mgx_extract_signal_*
entry point, the Python binding and the JavaScript facade use (include/meyda_gpu.h)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    capi.lib()
    return capi


def formula(S, n, hop):
    return 0 if S < n else (S - n) // hop + 1


@pytest.mark.parametrize("n", [256, 2048])
def test_signal_frames_matches_the_formula(capi, n):
    for hop in (1, 63, n // 4, n, n + 1, 5 * n):
        for S in (0, n - 1, n, n + 1, n + hop - 1, n + hop, 10 * n + 7):
            assert capi.signal_frames(S, n, hop) == formula(S, n, hop), (S, n, hop)


def test_signal_frames_64_bit(capi):
    assert capi.signal_frames(1 << 40, 1024, 1) == (1 << 40) - 1024 + 1
    assert capi.signal_frames((1 << 40) + 5, 2048, 4294967295) == formula((1 << 40) + 5, 2048, 4294967295)


def test_signal_frames_rejects_a_zero_hop_and_a_null_result(capi):
    L = capi.lib()
    f = ctypes.c_uint64(123)
    assert L.mgx_signal_frames(4096, 1024, 0, ctypes.byref(f)) == -1
    assert b"hop" in L.mgx_last_error()
    assert f.value == 123  # nothing written
    with pytest.raises(capi.MgxError) as e:
        capi.signal_frames(4096, 1024, 0)
    assert e.value.status == -1
    assert L.mgx_signal_frames(4096, 1024, 256, None) == -1
    assert L.mgx_last_error() != b""
    assert b"NULL" in L.mgx_last_error()


def test_signal_entry_points_validate_before_any_device_work(capi):
    """NULL plan or outputs: MGX_E_INVALID_ARGUMENT from every signal entry point, with no device touched."""
    L = capi.lib()
    o = capi.Outputs()
    assert L.mgx_extract_signal_device(None, None, 4096, 256, ctypes.byref(o), None) == -1
    assert L.mgx_extract_signal_host(None, None, 4096, 256, ctypes.byref(o)) == -1
    assert L.mgx_extract_signal_host_pcm(None, None, 0, 4096, 1, 2, 0, 256, ctypes.byref(o)) == -1
    assert L.mgx_last_error() != b""
