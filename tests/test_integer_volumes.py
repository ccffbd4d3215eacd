"""Integer (uint8 / int16 / uint16) volumes on the device pre-processing path, CPU half: the host side of the percentile
(ranks + numpy's interpolation) against np.percentile bit for bit, the truncated clip, and which volumes the routing
predicates of both deploy scripts send to the device."""
import numpy as np
import pytest

from ukbb_cardiac_amd import device_pipeline as dp

INT_DTYPES = [np.int16, np.uint16, np.uint8]


def _random(dtype, n, rng):
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=n, endpoint=True).astype(dtype)


def _host_percentile(a, q):
    """np.percentile through the helpers: exact order statistics (here from a sort) + the integer interpolation."""
    s = np.sort(a)
    k, k1, g = dp.percentile_ranks_int(a.size, q)
    return dp.lerp_like_numpy_int(s[k], s[k1], g, a.dtype)


@pytest.mark.parametrize('dtype', INT_DTYPES)
@pytest.mark.parametrize('n', [1, 2, 3, 101, 1000, 99991])
@pytest.mark.parametrize('q', [1, 99, 10.0, 0, 100, 37.5, 50])
def test_integer_percentile_helpers_equal_numpy(dtype, n, q):
    rng = np.random.default_rng(n * 7 + int(q * 10))
    a = _random(dtype, n, rng)
    if n > 10:
        a[rng.integers(0, n, size=n // 5)] = a[0]                 # ties
    got = _host_percentile(a, q)
    want = np.percentile(a, q)                                    # scalar q: for integer data also float64 quantiles
    assert got == want and type(got) is type(want) is np.float64
    got2 = (_host_percentile(a, q), _host_percentile(a, 50.0))
    want2 = np.percentile(a, (q, 50.0))                           # tuple q, as rescale_intensity passes it
    assert got2[0] == want2[0] and got2[1] == want2[1] and want2.dtype == np.float64


@pytest.mark.parametrize('dtype', INT_DTYPES)
def test_integral_virtual_index_and_narrow_ranges(dtype):
    """n - 1 a multiple of 100 (integral virtual indices at 1 % and 99 %) and a volume of only a few distinct values."""
    rng = np.random.default_rng(3)
    for n in (101, 201, 10001):
        a = _random(dtype, n, rng)
        k, _, g = dp.percentile_ranks_int(n, 1)
        assert g == 0.0 and k == (n - 1) // 100
        for q in ((1, 99), 1, 99, 10.0):
            want = np.percentile(a, q)
            got = [_host_percentile(a, v) for v in np.atleast_1d(q)]
            assert np.array_equal(np.atleast_1d(want), np.array(got))
    a = rng.integers(3, 6, size=5000).astype(dtype)
    assert _host_percentile(a, 1) == np.percentile(a, (1, 99))[0] and _host_percentile(a, 99) == np.percentile(a, (1, 99))[1]


def test_int16_interpolation_wraps_like_numpy():
    """numpy's _lerp subtracts the two neighbours in int16: neighbours more than 32767 apart wrap around, and the percentile can
    fall outside the data.  The helper reproduces that too."""
    a = np.array([-20000, 20000, 20000, 20000], np.int16)
    for q in ((1, 99), 10.0, 20.0):
        want = np.percentile(a, q)
        got = [_host_percentile(a, v) for v in np.atleast_1d(q)]
        assert np.array_equal(np.atleast_1d(want), np.array(got))
    assert np.percentile(a, 10.0) < -20000                        # the quirk is real under this numpy


@pytest.mark.parametrize('dtype', INT_DTYPES)
def test_clip_bounds_truncate_toward_zero(dtype):
    lo, hi = (-4.58, 3.7) if dtype == np.int16 else (0.58, 3.7)
    clo, chi = dp.clip_bounds_int(lo, hi, dtype)
    assert (clo, chi) == ((-4, 3) if dtype == np.int16 else (0, 3))
    img = np.arange(-7 if dtype == np.int16 else 0, 8).astype(dtype)
    ref = img.copy()
    ref[ref < np.float64(lo)] = np.float64(lo)                    # image_utils.rescale_intensity's in-place clip
    ref[ref > np.float64(hi)] = np.float64(hi)
    assert np.array_equal(dp.clip_like_reference(img, (np.float64(lo), np.float64(hi))), ref)
    assert ref.min() == clo and ref.max() == chi


class _FakeEngine:
    device = 0


def test_routing_predicates_admit_float32_and_the_three_integer_types(monkeypatch):
    from ukbb_cardiac_amd import deploy_network, deploy_network_ao
    checked = []
    monkeypatch.setattr(dp, 'device_zscore_matches_numpy', lambda engine, warn=None, dtype=np.float32: checked.append(np.dtype(dtype)) or True)
    admitted = {np.dtype(t) for t in (np.float32, np.uint8, np.int16, np.uint16)}
    all_types = [np.float32, np.float64, np.float16, np.uint8, np.int8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64]
    seq = deploy_network.define_flags().parse(['--seq_name', 'sa'])[0]
    ao = deploy_network_ao.define_flags().parse([])[0]
    eng = _FakeEngine()
    for t in all_types:
        img = np.zeros((4, 4, 1, 2), t)
        want = np.dtype(t) in admitted
        assert deploy_network.pipelined_on_device(img) == want, t
        assert deploy_network.sequence_on_device(seq, eng, img) == want, t
        assert deploy_network_ao.sequence_on_device(ao, eng, img, log=lambda *_: None) == want, t
        assert not deploy_network.sequence_on_device(seq, None, img)
        assert not deploy_network_ao.sequence_on_device(ao, None, img)
        assert not deploy_network.pipelined_on_device(np.zeros((4, 4, 2), t))
    assert checked == [np.dtype(t) for t in all_types if np.dtype(t) in admitted]   # the z-score self-check is keyed by dtype
    host = deploy_network.define_flags().parse(['--seq_name', 'sa', '--numpy1_casting'])[0]
    assert not deploy_network.sequence_on_device(host, eng, np.zeros((4, 4, 1, 2), np.int16))
    host = deploy_network.define_flags().parse(['--seq_name', 'sa', '--nodevice_preproc'])[0]
    assert not deploy_network.sequence_on_device(host, eng, np.zeros((4, 4, 1, 2), np.int16))
    host = deploy_network_ao.define_flags().parse(['--nodevice_preproc'])[0]
    assert not deploy_network_ao.sequence_on_device(host, eng, np.zeros((4, 4, 1, 2), np.int16))


def test_device_functions_still_refuse_other_dtypes():
    """float64 (any file with a non-trivial scl_slope), int32, int8: TypeError before anything touches a device."""
    for t in (np.float64, np.int32, np.int8, np.uint32):
        img = np.zeros((8, 8, 1, 2), t)
        for f in (lambda: dp.segment_sequence_device(img, _FakeEngine()), lambda: dp.aortic_sequence_device(img, _FakeEngine()),
                  lambda: dp.aortic_sequence_device(img, _FakeEngine(), window=(5, 0.1, 1))):
            with pytest.raises(TypeError):
                f()
