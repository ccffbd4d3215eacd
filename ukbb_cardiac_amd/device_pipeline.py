"""Sequence segmentation with the array handling of the deploy loop moved onto the GPU
(SURVEY.md section 8(f) row 3).

``segment_sequence_device`` produces exactly what ``pipeline.segment_sequence`` (the numpy mirror
of common/deploy_network.py:86-116) produces, but only two things cross PCIe per subject: the raw
float32 volume in, a uint8 label volume out.  The percentile sort of common/image_utils.py:72
(~20 M voxels per short-axis subject, the largest host cost of the reference loop) becomes an exact
4-pass radix select on the device, clip / rescale / pad / transpose one fused kernel, and the
label transposes plus the per-frame class counts of the ES pick (:125-130) another.

numpy's ``percentile(..., method='linear')`` is reproduced bit for bit: the device returns the two
neighbouring order statistics of each percentile, and the interpolation between them is done here
by numpy itself (``np.quantile`` on the two-element array with the same fractional index).

Volumes may be float32 or one of the integer types MR converters write (uint8, int16, uint16:
``NIFTI_DATATYPE``); integer volumes follow numpy's integer arithmetic (``*_int`` helpers below,
the ``*_t`` entry points of include/ukbb_fcn.h).  Any other dtype raises ``TypeError``.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .pipeline import pad_amounts, pad_amounts_fixed

# integer voxel types the device pre-processing takes, with their NIfTI datatype codes (those of ukbb_fcn_gzip_labels)
NIFTI_DATATYPE = {np.dtype(np.uint8): 2, np.dtype(np.int16): 4, np.dtype(np.uint16): 512}


def device_dtype_ok(dtype):
    """Is a volume of this dtype pre-processed on the device (float32 or one of NIFTI_DATATYPE)?"""
    return np.dtype(dtype) == np.float32 or np.dtype(dtype) in NIFTI_DATATYPE


def _check_dtype(image, host_alternative):
    if not device_dtype_ok(image.dtype):
        raise TypeError('device pre-processing is exact for float32, uint8, int16 and uint16 volumes only (got %s); use %s'
                        % (image.dtype, host_alternative))


def _to_device(image, dev):
    """Dense device copy of a host volume, strides preserved (a uint16 volume travels as int16: same bytes, a dtype torch has)."""
    import torch
    src = image if (image.flags.f_contiguous or image.flags.c_contiguous) else np.asfortranarray(image)
    if src.dtype == np.uint16:
        src = src.view(np.int16)
    return torch.from_numpy(src).to(dev)


def percentile_ranks(n, q):
    """0-based ranks (k, k+1) and the fractional part numpy's linear method uses for percentile q of n
    values when q is given as a tuple/array (as image_utils.py:72 does): float64 quantiles q/100,
    virtual index (n - 1) * quantile.  (A Python-scalar q on a float32 array takes a float32 path in
    numpy 2 and is not what the reference calls.)"""
    quantile = np.true_divide(np.float64(q), 100)
    virtual = (n - 1) * quantile
    k = int(math.floor(virtual))
    return k, min(k + 1, n - 1), np.float64(virtual - k)


def lerp_like_numpy(a_k, a_k1, gamma):
    """np.percentile's interpolation between the neighbouring order statistics a[k], a[k+1] (float32)."""
    # gamma goes in as a float64 ARRAY: numpy demotes scalar quantiles to the data's float32, which is not
    # the path a tuple of percentiles takes
    return np.quantile(np.array([a_k, a_k1], dtype=np.float32), np.array([gamma], dtype=np.float64))[0]


def percentile_ranks_int(n, q):
    """percentile_ranks for an INTEGER array: numpy divides q by the Python int 100 there (only float arrays get a divisor of
    their own dtype), so a scalar q and a tuple q both take float64 quantiles and a float64 virtual index (n - 1) * quantile --
    the float32 route of ``scalar_percentile_ranks`` does not exist for integer data.  Returns (k, k1, gamma) as numpy's
    _get_indexes / _get_gamma form them, including the top end: a virtual index >= n - 1 takes the last element (k = k1 =
    n - 1; gamma is then irrelevant, the two neighbours are equal)."""
    quantile = np.true_divide(q, 100)
    virtual = (n - 1) * quantile
    if virtual >= n - 1:
        return n - 1, n - 1, np.float64(0.0)
    k = int(math.floor(virtual))
    return k, k + 1, np.float64(virtual - k)


def lerp_like_numpy_int(a_k, a_k1, gamma, dtype):
    """np.percentile's interpolation between the neighbouring order statistics a[k] <= a[k+1] of an integer array: a float64
    result.  numpy's _lerp takes their difference IN THE INTEGER TYPE first (int16 neighbours more than 32767 apart wrap
    around), which numpy itself reproduces on the two-element array of that dtype with the same fractional index."""
    pair = np.array([a_k, a_k1], dtype=dtype)
    return np.quantile(pair, np.array([gamma], dtype=np.float64))[0]


def clip_bounds_int(lo, hi, dtype):
    """What image[image < lo] = lo / image[image > hi] = hi store into an integer array: the float64 bounds truncated toward
    zero (numpy's unsafe cast)."""
    b = np.array([lo, hi], dtype=np.float64).astype(dtype)
    return int(b[0]), int(b[1])


def _select(vol_t, dtype, ranks, stream, n=None):
    """The ranks-th smallest values of the first n (default: all) elements of a device tensor, in the volume's dtype
    (exact radix select)."""
    n = vol_t.numel() if n is None else n
    r = (C.c_uint64 * len(ranks))(*ranks)
    if np.dtype(dtype) == np.float32:
        out = np.empty(len(ranks), np.float32)
        _lib.check(_lib.lib.ukbb_fcn_select_kth(vol_t.data_ptr(), n, r, len(ranks), _lib.f32ptr(out), stream), 'ukbb_fcn_select_kth')
        return out
    out = np.empty(len(ranks), np.float64)
    _lib.check(_lib.lib.ukbb_fcn_select_kth_t(vol_t.data_ptr(), NIFTI_DATATYPE[np.dtype(dtype)], n, r, len(ranks),
                                              out.ctypes.data_as(C.POINTER(C.c_double)), stream), 'ukbb_fcn_select_kth_t')
    return out.astype(dtype)


def device_percentiles(vol_t, qs, stream=0, dtype=np.float32, n=None):
    """Exact np.percentile(volume, qs) of a dense torch tensor on the GPU; ``dtype``: the host volume's dtype (float32, or
    an integer type of NIFTI_DATATYPE -- a uint16 volume is an int16 tensor on the device); ``n``: the number of voxels when
    the volume fills only the start of the tensor (a staging buffer, whatever its torch dtype)."""
    n = vol_t.numel() if n is None else n
    integer = np.dtype(dtype) != np.float32
    ranks, gammas = [], []
    for q in qs:
        k, k1, g = percentile_ranks_int(n, q) if integer else percentile_ranks(n, q)
        ranks += [k, k1]
        gammas.append(g)
    out = _select(vol_t, dtype, ranks, stream, n)
    if integer:
        return [lerp_like_numpy_int(out[2 * i], out[2 * i + 1], gammas[i], dtype) for i in range(len(qs))]
    return [lerp_like_numpy(out[2 * i], out[2 * i + 1], gammas[i]) for i in range(len(qs))]


def pack_rescaled(vol_ptr, dtype, shape, strides, lo, hi, pad, batch_ptr, stream):
    """Clip + rescale + pad + transpose of a device (X,Y,Z,T) volume (element strides) into the network batch [T*Z][X2][Y2]:
    ukbb_fcn_rescale_pack, or for an integer volume ukbb_fcn_rescale_pack_t with the truncated clip bounds.
    pad = (X2, Y2, x_pre, y_pre)."""
    if np.dtype(dtype) == np.float32:
        _lib.check(_lib.lib.ukbb_fcn_rescale_pack(vol_ptr, *shape, *strides, float(lo), float(hi), *pad, batch_ptr, stream),
                   'ukbb_fcn_rescale_pack')
        return
    clo, chi = clip_bounds_int(lo, hi, dtype)
    _lib.check(_lib.lib.ukbb_fcn_rescale_pack_t(vol_ptr, NIFTI_DATATYPE[np.dtype(dtype)], *shape, *strides, clo, chi, float(lo), float(hi),
                                                *pad, batch_ptr, stream), 'ukbb_fcn_rescale_pack_t')


def forward_chunks(engine, batch_ptr, pred_ptr, n, X2, Y2, batch_slices, stream, chunk_stats=()):
    """The frame-wise network over the packed batch [n][X2][Y2] at batch_ptr in chunks of batch_slices, enqueued on ``stream``: int32
    label maps to pred_ptr.  chunk_stats: [(statistic, work_ptr, out_ptr, shape, pad)] of the statistics that read the probabilities
    (``per_chunk``: ConfidenceStats).  With one, every chunk's forward also stores its probabilities -- into the statistic's work buffer,
    one chunk large, written again by the next chunk -- and the statistic's launch is queued behind the chunk on the same stream."""
    engine.reserve(min(batch_slices, n), X2, Y2)
    prob_ptr = chunk_stats[0][1] if chunk_stats else 0
    for i in range(0, n, batch_slices):
        m = min(batch_slices, n - i)
        engine.run_device(batch_ptr + 4 * i * X2 * Y2, m, X2, Y2, prob_ptr=prob_ptr, pred_ptr=pred_ptr + 4 * i * X2 * Y2, stream=stream)
        for stat, _, out_ptr, shape, pad in chunk_stats:
            stat.launch_chunk(prob_ptr, pred_ptr + 4 * i * X2 * Y2, m, i, shape, pad, engine.arch.n_class, out_ptr, stream)


def forward_and_unpack(engine, batch_ptr, pred_ptr, shape, pad, batch_slices, lab_ptr, counts_ptr, stream, chunk_stats=()):
    """The tail every frame-wise sequence path shares, enqueued on ``stream``: the network over the packed batch [T*Z][X2][Y2] at
    batch_ptr in chunks of batch_slices (int32 label maps to pred_ptr), then ukbb_fcn_unpack_labels: the uint8 (X,Y,Z,T) label
    volume in NIfTI order to lab_ptr and the per-frame class counts (int64 [T, n_class]) to counts_ptr.  pad = (X2, Y2, x_pre, y_pre).
    chunk_stats: [(statistic, work_ptr, out_ptr)] of the per-chunk statistics (forward_chunks), their outputs zeroed by the caller."""
    X, Y, Z, T = shape
    X2, Y2, x_pre, y_pre = pad
    forward_chunks(engine, batch_ptr, pred_ptr, T * Z, X2, Y2, batch_slices, stream,
                   [(stat, work_ptr, out_ptr, shape, pad) for stat, work_ptr, out_ptr in chunk_stats])
    _lib.check(_lib.lib.ukbb_fcn_unpack_labels(pred_ptr, X, Y, Z, T, X2, Y2, x_pre, y_pre, engine.arch.n_class, lab_ptr, counts_ptr, stream),
               'ukbb_fcn_unpack_labels')


def segment_sequence_device(image, engine, batch_slices=128, thres=(1, 99), return_aux=False, stats=(), stat_args=None):
    """(X,Y,Z,T) float32 / uint8 / int16 / uint16 volume -> float64 label volume of the same shape, like
    pipeline.segment_sequence.

    ``image`` is NOT modified (the reference clips it in place); callers that
    save image frames afterwards clip them with the returned bounds (``aux['clip']``: the float64
    percentiles; clip_like_reference stores them into an integer frame truncated, as numpy does).
    ``aux['counts'][t, c]`` = voxels of class c in frame t (input of the ES pick).  ``stats`` (needs ``return_aux``): label
    statistics (GateStats, AtrialStats, ScoreStats; ConfidenceStats: from the probabilities, chunk by chunk) to compute while the labels are still on the device, ``stat_args`` their
    per-subject arguments {key: arg}: ``aux['stats']`` = {key: decoded statistic} (label_statistics)."""
    import torch
    if stats and not return_aux:
        raise ValueError('stats are returned in aux: pass return_aux')
    if image.ndim != 4:
        raise ValueError('expected a 4-D (X,Y,Z,T) sequence, got shape %s' % (image.shape,))
    _check_dtype(image, 'pipeline.segment_sequence')
    dev = torch.device('cuda', engine.device)
    vol = _to_device(image, dev)                                 # dense copy, strides preserved
    return segment_sequence_tensor(vol, image.dtype, image.shape, engine, batch_slices, thres, return_aux, stats, stat_args)


def segment_sequence_tensor(vol_t, dtype, shape, engine, batch_slices=128, thres=(1, 99), return_aux=False, stats=(), stat_args=None):
    """segment_sequence_device for a volume that is on the device already (device_inflate.DeviceInflater: the voxels never were
    on the host): ``vol_t`` a 4-D torch tensor of ``shape`` (X,Y,Z,T) on the engine's device, dense (a permutation of contiguous memory, in any stride order), holding voxels of the
    numpy ``dtype`` (a uint16 volume is an int16 tensor).  Same results, same exceptions."""
    import torch
    if stats and not return_aux:
        raise ValueError('stats are returned in aux: pass return_aux')
    if len(shape) != 4 or tuple(vol_t.shape) != tuple(shape):
        raise ValueError('expected a 4-D (X,Y,Z,T) sequence, got shape %s' % (tuple(shape),))
    if not device_dtype_ok(dtype):
        raise TypeError('device pre-processing is exact for float32, uint8, int16 and uint16 volumes only (got %s); use %s'
                        % (np.dtype(dtype), 'pipeline.segment_sequence'))
    X, Y, Z, T = (int(v) for v in shape)
    dev = torch.device('cuda', engine.device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lo, hi = device_percentiles(vol_t, thres, stream, dtype)
    X2, Y2, x_pre, _, y_pre, _ = pad_amounts(X, Y)
    n = T * Z
    batch = torch.empty((n, X2, Y2), dtype=torch.float32, device=dev)
    sx, sy, sz, st = vol_t.stride()
    pack_rescaled(vol_t.data_ptr(), dtype, (X, Y, Z, T), (sx, sy, sz, st), lo, hi, (X2, Y2, x_pre, y_pre), batch.data_ptr(), stream)
    pred = torch.empty((n, X2, Y2), dtype=torch.int32, device=dev)
    n_class = engine.arch.n_class
    lab = torch.empty(X * Y * Z * T, dtype=torch.uint8, device=dev)
    counts = torch.empty((T, n_class), dtype=torch.int64, device=dev)
    per_chunk = chunk_statistics_buffers(stats, (X, Y, Z, T), n_class, dev)
    forward_and_unpack(engine, batch.data_ptr(), pred.data_ptr(), (X, Y, Z, T), (X2, Y2, x_pre, y_pre), batch_slices, lab.data_ptr(),
                       counts.data_ptr(), stream, [(stat, work.data_ptr(), out.data_ptr()) for stat, work, out in per_chunk])
    lab_h = lab.cpu().numpy().reshape((X, Y, Z, T), order='F')
    out = np.zeros((X, Y, Z, T))                                # float64, as deploy_network.py:92
    out[...] = lab_h
    if return_aux:
        aux = {'clip': (lo, hi), 'counts': counts.cpu().numpy()}
        aux['stats'] = label_statistics(lab, (X, Y, Z, T), n_class, stats, stat_args, stream, aux['counts'])
        for stat, _, d_out in per_chunk:
            aux['stats'][stat.key] = stat.decode(d_out.cpu().numpy(), (X, Y, Z, T), n_class, aux['counts'])
        return out, aux
    return out


def clip_like_reference(frame, clip):
    """What a frame of ``image`` holds after the reference's in-place clip (image_utils.py:73-74)."""
    lo, hi = clip
    f = np.array(frame, copy=True)
    f[f < lo] = lo
    f[f > hi] = hi
    return f


def pick_ed_es_from_counts(counts, seq_name, seg4=False):
    """pipeline.pick_ed_es on the per-frame class counts (deploy_network.py:125-130)."""
    c1 = counts[:, 1]
    if seq_name == 'sa' or (seq_name == 'la_4ch' and seg4):
        return 0, int(np.argmin(c1))
    return 0, int(np.argmax(c1))


# ---- aortic cine: z-score + UNet-LSTM on the device (common/deploy_network_ao.py:92-107,129-189) ------------------

def scalar_percentile_ranks(n, q):
    """0-based ranks (k, k+1) and the float32 fractional part np.percentile uses when q is a Python SCALAR and the data
    float32 (image_utils.py:62, ``np.percentile(image, thres_roi)``): numpy 2 then keeps everything in the data's
    dtype -- quantile = q / float32(100), virtual index (n - 1) * quantile in float32, gamma = float32(float64(virtual) - k)."""
    quantile = np.true_divide(q, np.float32(100))
    virtual = np.asanyarray((n - 1) * quantile)
    if virtual >= n - 1:
        return n - 1, n - 1, 0.0
    k = int(np.floor(virtual))
    gamma = np.asanyarray(np.asanyarray(virtual - np.asanyarray(k, dtype=np.intp)), dtype=virtual.dtype)
    return k, k + 1, float(gamma)


def device_scalar_percentile(vol_t, q, stream=0):
    """Exact np.percentile(float32 volume, q) for a Python-scalar q, on the device."""
    n = vol_t.numel()
    k, k1, g = scalar_percentile_ranks(n, q)
    r = (C.c_uint64 * 2)(k, k1)
    out = np.empty(2, np.float32)
    _lib.check(_lib.lib.ukbb_fcn_select_kth(vol_t.data_ptr(), n, r, 2, _lib.f32ptr(out), stream), 'ukbb_fcn_select_kth')
    # numpy's own float32 lerp: a Python-float quantile on a float32 array stays float32, (2 - 1) * g = g exactly
    return np.quantile(out, g)


def device_zscore_stats(vol_t, thres_roi=10.0, stream=0, dtype=np.float32):
    """(mu, sigma + eps, n_roi, val_l) of image_utils.normalise_intensity for a dense (X,Y,Z,T) torch tensor on the
    GPU, bit-identical to numpy: the ROI is compacted in numpy's element order and summed along numpy's pairwise tree
    (``ukbb_fcn_roi_compact`` / ``ukbb_fcn_pairwise_sum``); the few scalar operations around the sums are numpy's own.
    ``dtype``: the host volume's dtype.  float32: float32 sums and results, as numpy.  An integer type of NIFTI_DATATYPE:
    float64 threshold, float64 sums (the plain one exact), float64 mu and sigma + eps (the ``*_t`` entry points)."""
    import torch
    if np.dtype(dtype) != np.float32:
        return _device_zscore_stats_int(vol_t, thres_roi, stream, np.dtype(dtype))
    X, Y, Z, T = vol_t.shape
    val_l = device_scalar_percentile(vol_t, thres_roi, stream)
    roi = torch.empty(vol_t.numel(), dtype=torch.float32, device=vol_t.device)
    sx, sy, sz, st = vol_t.stride()
    n_roi = C.c_uint64(0)
    _lib.check(_lib.lib.ukbb_fcn_roi_compact(vol_t.data_ptr(), X, Y, Z, T, sx, sy, sz, st, float(val_l), roi.data_ptr(),
                                             C.byref(n_roi), stream), 'ukbb_fcn_roi_compact')
    n = np.intp(n_roi.value)                                  # _count_reduce_items returns an intp scalar: the divisions below are float64
    s = C.c_float(0)
    _lib.check(_lib.lib.ukbb_fcn_pairwise_sum(roi.data_ptr(), int(n), 0, 0.0, C.byref(s), stream), 'ukbb_fcn_pairwise_sum')
    with np.errstate(all='ignore'):
        mu = np.float32(np.float32(s.value) / n)             # np.mean: ret.dtype.type(ret / rcount)
        _lib.check(_lib.lib.ukbb_fcn_pairwise_sum(roi.data_ptr(), int(n), 1, float(mu), C.byref(s), stream), 'ukbb_fcn_pairwise_sum')
        var = np.float32(np.float32(s.value) / n)            # np.var: sum((x - mean)^2) in float32, / n in float64, back to float32
        sigma = np.float32(np.sqrt(var))
    return mu, sigma + 1e-6, int(n), val_l                   # float32 + Python float stays float32 (image_utils.py:66-67)


def _device_zscore_stats_int(vol_t, thres_roi, stream, dtype):
    """device_zscore_stats of an integer volume.  numpy there: val_l = float64 percentile (float64 quantile whether q is a
    scalar or not), roi = image >= val_l compared in float64, np.mean / np.std reduce with dtype float64 -- the plain sum of
    8/16-bit values is exact in any order (every partial sum an integer below 2^53), the sum of (x - mu)^2 follows numpy's
    pairwise tree -- and divide by the intp count: everything float64."""
    import torch
    X, Y, Z, T = vol_t.shape
    code = NIFTI_DATATYPE[dtype]
    n_all = vol_t.numel()
    k, k1, g = percentile_ranks_int(n_all, thres_roi)
    a = _select(vol_t, dtype, [k, k1], stream)
    val_l = lerp_like_numpy_int(a[0], a[1], g, dtype)
    roi = torch.empty(n_all, dtype=vol_t.dtype, device=vol_t.device)
    sx, sy, sz, st = vol_t.stride()
    n_roi = C.c_uint64(0)
    _lib.check(_lib.lib.ukbb_fcn_roi_compact_t(vol_t.data_ptr(), code, X, Y, Z, T, sx, sy, sz, st, float(val_l), roi.data_ptr(),
                                               C.byref(n_roi), stream), 'ukbb_fcn_roi_compact_t')
    n = np.intp(n_roi.value)
    s = C.c_double(0)
    _lib.check(_lib.lib.ukbb_fcn_pairwise_sum_t(roi.data_ptr(), code, int(n), 0, 0.0, C.byref(s), stream), 'ukbb_fcn_pairwise_sum_t')
    with np.errstate(all='ignore'):
        mu = np.float64(np.float64(s.value) / n)              # np.mean: float64 sum / intp count
        _lib.check(_lib.lib.ukbb_fcn_pairwise_sum_t(roi.data_ptr(), code, int(n), 1, float(mu), C.byref(s), stream),
                   'ukbb_fcn_pairwise_sum_t')
        var = np.float64(np.float64(s.value) / n)             # np.var: float64 sum of squared deviations / intp count
        sigma = np.sqrt(var)
    return mu, sigma + 1e-6, int(n), val_l


def zscore_pack(vol_ptr, dtype, shape, strides, mu, den, pad, batch_ptr, stream):
    """(v - mu) / den + pad + transpose of a device (X,Y,Z,T) volume into [T*Z][X2][Y2]: ukbb_fcn_zscore_pack (float32
    arithmetic) or, for an integer volume, ukbb_fcn_zscore_pack_t (float64 arithmetic).  pad = (X2, Y2, x_pre, y_pre)."""
    if np.dtype(dtype) == np.float32:
        _lib.check(_lib.lib.ukbb_fcn_zscore_pack(vol_ptr, *shape, *strides, float(mu), float(den), *pad, batch_ptr, stream),
                   'ukbb_fcn_zscore_pack')
        return
    _lib.check(_lib.lib.ukbb_fcn_zscore_pack_t(vol_ptr, NIFTI_DATATYPE[np.dtype(dtype)], *shape, *strides, float(mu), float(den),
                                               *pad, batch_ptr, stream), 'ukbb_fcn_zscore_pack_t')


_ZSCORE_OK = {}


def _zscore_probe(dtype):
    """A 26 k-voxel probe volume of the dtype: more than three reduction buffers, ROI not a multiple of anything, ties."""
    rng = np.random.default_rng(20261003)
    probe = 1000.0 * rng.gamma(2.0, 1.0, size=(37, 29, 1, 25))
    if dtype == np.float32:
        return probe.astype(np.float32)
    info = np.iinfo(dtype)
    scale = 1.0 if info.max > 10000 else 0.05                   # uint8: squeeze into 0..255 (many ties)
    if dtype == np.int16:
        probe -= 300.0                                          # negative intensities too
    return np.clip(np.round(probe * scale), info.min, info.max).astype(dtype)


def device_zscore_matches_numpy(engine, warn=None, dtype=np.float32):
    """Once per process, device and dtype: does the device z-score reproduce THIS numpy?  ``device_zscore_stats`` mirrors numpy
    internals -- the 8192-element buffering and the 128-element / 8-accumulator pairwise leaves of ``np.add.reduce``, the float32
    handling of a scalar percentile, the float64 reductions of integer data -- that ``np.setbufsize`` or another numpy release
    can change without notice.  A 26 k-voxel probe of the dtype is pushed through both; on any difference in
    (val_l, mu, sigma + eps) the callers keep the host path (deploy_network_ao.py) and say so."""
    dtype = np.dtype(dtype)
    key = (engine.device, dtype)
    if key not in _ZSCORE_OK:
        import torch
        ok, why = True, ''
        if not device_dtype_ok(dtype):
            ok, why = False, 'no device z-score for %s volumes' % dtype
        elif np.getbufsize() != 8192:
            ok, why = False, 'np.getbufsize() = %d, the device reproduces the 8192-element default' % np.getbufsize()
        else:
            probe = _zscore_probe(dtype)
            val_l = np.percentile(probe, 10.0)
            roi = probe[probe >= val_l]
            want = (val_l, np.mean(roi), np.std(roi) + 1e-6)
            dev = torch.device('cuda', engine.device)
            vol = _to_device(np.asfortranarray(probe), dev)
            mu, den, _, got_l = device_zscore_stats(vol, 10.0, torch.cuda.current_stream(dev).cuda_stream, dtype)
            got = (got_l, mu, den)
            rt = np.float32 if dtype == np.float32 else np.float64
            if not all(rt(a) == rt(b) for a, b in zip(want, got)):
                ok, why = False, 'probe statistics differ for %s: numpy %r, device %r (numpy %s)' % (dtype, want, got, np.__version__)
        _ZSCORE_OK[key] = (ok, why)
        if not ok and warn is not None:
            warn('  device z-score disabled, host pre-processing used instead: ' + why)
    return _ZSCORE_OK[key][0]


def device_qc_stats(vol_t, lab_t, dtype, n_class, stream=0, min_size=None):
    """The three statistics of aorta_qc (``n_large``, ``max``, ``mean_ed``: see that module) of the dense (X,Y,Z,T) torch
    cine ``vol_t`` (``dtype``: the host volume's dtype; a uint16 cine is an int16 tensor) and the uint8 labels ``lab_t`` in NIfTI
    order that ukbb_fcn_unpack_labels left on the device, equal to aorta_qc.stats_host of the same arrays.  Components and
    maxima: ukbb_fcn_label_components / ukbb_fcn_label_max; the mean: ukbb_fcn_label_compact + numpy's pairwise tree
    (ukbb_fcn_pairwise_sum / _t) and numpy's division, as device_zscore_stats."""
    import torch
    from .aorta_qc import PIXEL_THRES
    min_size = PIXEL_THRES if min_size is None else min_size
    X, Y, Z, T = vol_t.shape
    dtype = np.dtype(dtype)
    code = 16 if dtype == np.float32 else NIFTI_DATATYPE[dtype]
    sx, sy, sz, st = vol_t.stride()
    work = torch.empty(2 * X * Y * Z * T, dtype=torch.int32, device=vol_t.device)
    n_large = torch.empty((T, n_class), dtype=torch.int32, device=vol_t.device)
    _lib.check(_lib.lib.ukbb_fcn_label_components(lab_t.data_ptr(), X, Y, Z, T, n_class, min_size, work.data_ptr(), n_large.data_ptr(),
                                                  stream), 'ukbb_fcn_label_components')
    mx = torch.empty((T, n_class), dtype=torch.float64, device=vol_t.device)
    _lib.check(_lib.lib.ukbb_fcn_label_max(vol_t.data_ptr(), code, X, Y, Z, T, sx, sy, sz, st, lab_t.data_ptr(), n_class, mx.data_ptr(),
                                           stream), 'ukbb_fcn_label_max')
    comp = torch.empty(X * Y * Z, dtype=vol_t.dtype, device=vol_t.device)
    rt = np.float32 if dtype == np.float32 else np.float64        # numpy's .mean() result type (float64 for integer data)
    means = [rt(np.nan)]
    for k in range(1, n_class):
        n_k = C.c_uint64(0)
        _lib.check(_lib.lib.ukbb_fcn_label_compact(vol_t.data_ptr(), code, X, Y, Z, sx, sy, sz, lab_t.data_ptr(), k, comp.data_ptr(),
                                                   C.byref(n_k), stream), 'ukbb_fcn_label_compact')
        n = np.intp(n_k.value)                                     # _count_reduce_items: an intp count
        if dtype == np.float32:
            s = C.c_float(0)
            _lib.check(_lib.lib.ukbb_fcn_pairwise_sum(comp.data_ptr(), int(n), 0, 0.0, C.byref(s), stream), 'ukbb_fcn_pairwise_sum')
        else:
            s = C.c_double(0)
            _lib.check(_lib.lib.ukbb_fcn_pairwise_sum_t(comp.data_ptr(), code, int(n), 0, 0.0, C.byref(s), stream), 'ukbb_fcn_pairwise_sum_t')
        with np.errstate(all='ignore'):
            means.append(rt(rt(s.value) / n))                      # np.mean: ret.dtype.type(ret / rcount); empty: 0 / 0 = NaN
    return {'n_large': n_large.cpu().numpy(), 'max': mx.cpu().numpy(), 'mean_ed': np.array(means, dtype=rt)}


# ---- statistics of the label volume ukbb_fcn_unpack_labels left in HBM: the gates (qc_gates.py), the atria (atrial.py), the score against a
# second segmentation (seg_score.py) -----------------------------------------------------------------------------------------------------
# A statistic has a ``key``, says whether it takes a per-subject argument (``needs_arg``), and knows the (work, out) int32 counts
# of its device buffers (``sizes``), how to enqueue itself on a stream (``launch``; the work buffer 8-byte aligned; asynchronous)
# and how to read the host copy of what it wrote (``decode``).  SubjectPipeline keeps such buffers per slot; label_statistics
# allocates them per call.

class GateStats:
    """qc_gates.stats_host -- what the gate of this sequence reads (the input of qc_gates.gate_from_stats) -- of an (X,Y,Z,T) label
    volume: ukbb_fcn_plane_components for sa (the Z planes of frame 0) and la_4ch --seg4 (plane 0), ukbb_fcn_label_components for
    the atrial gate (the whole sequence).  plane_args = (a, b, keep_min) of the plane statistics (qc_gates.plane_stats_host)."""
    key, needs_arg, per_chunk = 'qc', False, False

    def __init__(self, seq_name, seg4, plane_args=None):
        from .qc_gates import PIXEL_THRES, gate_kind
        self.kind = gate_kind(seq_name, seg4)
        self.plane_args = (1, 2, PIXEL_THRES) if plane_args is None else plane_args
        self.min_size = PIXEL_THRES

    def sizes(self, shape, n_class):
        X, Y, Z, T = shape
        if self.kind == 'atrium':
            return 2 * X * Y * Z * T, T * n_class
        P = Z if self.kind == 'sa' else 1
        return 2 * P * n_class + 3 * X * Y * P + (X * Y * P + 3) // 4, P * (3 * n_class + 1)

    def launch(self, lab_ptr, shape, n_class, work_ptr, out_ptr, stream, arg=None):
        X, Y, Z, T = shape
        if self.kind == 'atrium':
            _lib.check(_lib.lib.ukbb_fcn_label_components(lab_ptr, X, Y, Z, T, n_class, self.min_size, work_ptr, out_ptr, stream),
                       'ukbb_fcn_label_components')
            return
        P = Z if self.kind == 'sa' else 1                             # frame 0 comes first in NIfTI order, plane 0 first in it
        cells = 4 * P * n_class
        _lib.check(_lib.lib.ukbb_fcn_plane_components(lab_ptr, X, Y, P, n_class, *self.plane_args, work_ptr, out_ptr, out_ptr + cells,
                                                      out_ptr + 2 * cells, out_ptr + 3 * cells, stream), 'ukbb_fcn_plane_components')

    def decode(self, out, shape, n_class, counts=None):
        """The atrial gate also takes the per-frame class counts of ukbb_fcn_unpack_labels."""
        X, Y, Z, T = shape
        out = np.asarray(out, dtype=np.int32)
        if self.kind == 'atrium':
            return {'counts': np.asarray(counts), 'n_large': out[:T * n_class].reshape(T, n_class).copy()}
        P = Z if self.kind == 'sa' else 1
        c = P * n_class
        return {'count': out[:c].reshape(P, n_class).copy(), 'largest': out[c:2 * c].reshape(P, n_class).copy(),
                'kept': out[2 * c:3 * c].reshape(P, n_class).copy(), 'union_largest': out[3 * c:3 * c + P].copy()}


class AtrialStats:
    """atrial.frame_stats_host, [T, n_class, 8], of an (X,Y,1,T) label volume (one slice: every frame a plane of
    ukbb_fcn_atrial_area_length).  Per-subject argument: (affine, long_axis) -- the voxel-to-world matrix of the long-axis image and
    atrial.long_axis_from_sa; only the T*n_class*32 bytes of statistics cross to the host."""
    key, needs_arg, per_chunk = 'atrial', True, False

    def sizes(self, shape, n_class):
        X, Y, Z, T = shape
        return 2 * T * n_class + 3 * X * Y * T + (X * Y * T + 3) // 4, T * n_class * 8

    def launch(self, lab_ptr, shape, n_class, work_ptr, out_ptr, stream, arg):
        X, Y, Z, T = shape
        if Z != 1:
            raise ValueError('the atrial measures read a single-slice long-axis sequence, got Z = %d' % Z)
        affine, long_axis = arg
        a = (C.c_double * 12)(*[float(v) for v in np.asarray(affine, np.float64)[:3, :4].ravel()])
        l = (C.c_double * 3)(*[float(v) for v in np.asarray(long_axis, np.float64).ravel()[:3]])
        _lib.check(_lib.lib.ukbb_fcn_atrial_area_length(lab_ptr, X, Y, T, n_class, a, l, work_ptr, out_ptr, stream), 'ukbb_fcn_atrial_area_length')

    def decode(self, out, shape, n_class, counts=None):
        T = shape[3]
        return np.asarray(out, dtype=np.int32)[:T * n_class * 8].reshape(T, n_class, 8).copy()


class ScoreStats:
    """seg_score.stats_host -- overlap counts and contour distances per (plane, class) -- of an (X,Y,Z,T) label volume against a second
    one (ukbb_fcn_score_planes).  Per-subject argument: the truth volume, a uint8 (X,Y,Z,T) array; it is uploaded once, on the
    stream the statistic is enqueued on, and only the Z*T*n_class*48 bytes of results cross back.  A plane larger than the kernel's
    bit planes hold (``fits``) is for seg_score.stats_host."""
    key, needs_arg, per_chunk = 'score', True, False

    def __init__(self, device=None):
        self.device = device                                          # of the label volume; None: torch's current device

    @staticmethod
    def fits(shape, n_class):
        X, Y, Z, T = shape
        return Z * T <= 65535 and int(_lib.lib.ukbb_fcn_score_planes_work(X, Y, Z * T, max(2, n_class))) > 0

    def sizes(self, shape, n_class):
        X, Y, Z, T = shape
        P = Z * T
        return (int(_lib.lib.ukbb_fcn_score_planes_work(X, Y, P, max(2, n_class))) + 3) // 4, P * n_class * 12

    def launch(self, lab_ptr, shape, n_class, work_ptr, out_ptr, stream, arg):
        import contextlib
        import torch
        X, Y, Z, T = shape
        truth = np.asarray(arg)
        if truth.dtype != np.uint8 or truth.shape != tuple(shape):
            raise ValueError('the truth volume is a uint8 array of the shape of the labels %s, got %s %s' % (tuple(shape), truth.dtype, truth.shape))
        flat = np.asfortranarray(truth).reshape(-1, order='F')
        # torch's allocator ties the block to the stream current at the allocation: freed behind the launch, it is handed out again
        # only in stream order
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.device)) if stream else contextlib.nullcontext():
            d_truth = torch.from_numpy(flat).to(torch.device('cuda', torch.cuda.current_device() if self.device is None else self.device))
            P = Z * T
            _lib.check(_lib.lib.ukbb_fcn_score_planes(lab_ptr, d_truth.data_ptr(), X, Y, P, n_class, work_ptr, out_ptr, out_ptr + 32 * P * n_class,
                                                      stream), 'ukbb_fcn_score_planes')

    def decode(self, out, shape, n_class, counts=None):
        P = shape[2] * shape[3]
        out = np.ascontiguousarray(np.asarray(out, dtype=np.int32)[:P * n_class * 12])
        return {'shape': tuple(int(v) for v in shape), 'cells': out[:P * n_class * 8].reshape(P, n_class, 8).copy(),
                'sums': out[P * n_class * 8:].view(np.float64).reshape(P, n_class, 2).copy()}


class ConfidenceStats:
    """confidence.cells_host -- [T, n_class, 20] uint64 reductions of the softmax per (frame, class) -- of a subject
    (ukbb_fcn_confidence_cells).  It reads what the other statistics never see, the probabilities, and they exist for one chunk of slices
    at a time: ``per_chunk``.  Its work buffer is that chunk's probabilities [batch_slices][X2][Y2][n_class] float32, which the forward
    fills (forward_chunks); ``launch_chunk`` adds the chunk into the cells, which the caller has zeroed; only the T*n_class*160 bytes of
    cells cross to the host.  pad(X, Y) -> (X2, Y2, x_pre, _, y_pre, _): how the path pads its batch; n_class: the model's, where the
    caller sizes buffers for any model."""
    key, needs_arg, per_chunk = 'confidence', False, True

    def __init__(self, batch_slices, n_class=None, pad=pad_amounts):
        self.batch_slices, self.n_class, self.pad = int(batch_slices), n_class, pad

    def sizes(self, shape, n_class):
        X, Y, Z, T = shape
        X2, Y2 = self.pad(X, Y)[:2]
        C = self.n_class or n_class
        return min(self.batch_slices, Z * T) * X2 * Y2 * C, T * C * 40

    def launch(self, lab_ptr, shape, n_class, work_ptr, out_ptr, stream, arg=None):
        raise RuntimeError('ConfidenceStats reads the probabilities of a chunk of slices: launch_chunk, behind the chunk\'s forward')

    def launch_chunk(self, prob_ptr, pred_ptr, n, first_slice, shape, pad, n_class, out_ptr, stream):
        X, Y, Z, T = shape
        _lib.check(_lib.lib.ukbb_fcn_confidence_cells(prob_ptr, pred_ptr, n, X, Y, Z, T, *pad, n_class, first_slice, out_ptr, stream),
                   'ukbb_fcn_confidence_cells')

    def decode(self, out, shape, n_class, counts=None):
        T = shape[3]
        return np.ascontiguousarray(np.asarray(out, dtype=np.int32)[:T * n_class * 40]).view(np.uint64).reshape(T, n_class, 20).copy()


def chunk_statistics_buffers(stats, shape, n_class, device):
    """[(statistic, work, out)] for the per-chunk statistics among ``stats``: fresh device tensors, the output zeroed on the current stream."""
    import torch
    got = []
    for stat in stats:
        if stat.per_chunk:
            n_work, n_out = stat.sizes(shape, n_class)
            got.append((stat, torch.empty(n_work, dtype=torch.float32, device=device), torch.zeros(n_out, dtype=torch.int32, device=device)))
    return got


def stat_skipped(stat, stat_args):
    """A statistic that takes a per-subject argument and has none for this subject (a long-axis subject without sa.nii.gz) is not
    computed for it."""
    return stat.needs_arg and (stat_args or {}).get(stat.key) is None


def label_statistics(lab_t, shape, n_class, stats, stat_args=None, stream=0, counts=None):
    """{key: decoded statistic} of the (X,Y,Z,T) uint8 label volume ``lab_t`` (a device tensor, NIfTI order) for a sequence of
    statistics: buffers, launch, copy to the host and decode, one statistic after the other.  stat_args: {key: per-subject argument};
    counts: the per-frame class counts of ukbb_fcn_unpack_labels, for the decodes that read them."""
    import torch
    got = {}
    for stat in stats:
        if stat.per_chunk or stat_skipped(stat, stat_args):       # per-chunk statistics ran with the forward (forward_chunks)
            continue
        n_work, n_out = stat.sizes(shape, n_class)
        work = torch.empty(n_work, dtype=torch.int32, device=lab_t.device)
        out = torch.empty(n_out, dtype=torch.int32, device=lab_t.device)
        stat.launch(lab_t.data_ptr(), shape, n_class, work.data_ptr(), out.data_ptr(), stream, (stat_args or {}).get(stat.key))
        got[stat.key] = stat.decode(out.cpu().numpy(), shape, n_class, counts)
    return got


def device_plane_stats(lab_t, X, Y, P, n_class, a=1, b=2, keep_min=10, stream=0):
    """qc_gates.plane_stats_host of the first P planes of X*Y uint8 labels (x fastest) of a device tensor:
    ukbb_fcn_plane_components."""
    return label_statistics(lab_t, (X, Y, P, 1), n_class, [GateStats('sa', False, (a, b, keep_min))], stream=stream)['qc']


def device_gate_stats(lab_t, shape, seq_name, seg4, n_class, stream=0, counts=None):
    """qc_gates.stats_host of the (X,Y,Z,T) uint8 label volume ``lab_t`` (NIfTI order) on the device.  ``counts``: the per-frame
    class counts if the caller has them (ukbb_fcn_unpack_labels, as on every path of the deploy script); the atrial gate
    otherwise takes them from one torch.bincount over the label tensor."""
    import torch
    X, Y, Z, T = shape
    gate = GateStats(seq_name, seg4)
    if gate.kind == 'atrium' and counts is None:
        # one histogram over (frame, label) keys; labels >= n_class fall into columns that are dropped
        keys = lab_t[:X * Y * Z * T].view(T, -1).to(torch.int64) + 256 * torch.arange(T, device=lab_t.device)[:, None]
        counts = torch.bincount(keys.reshape(-1), minlength=256 * T).view(T, 256)[:, :n_class].cpu().numpy()
    return label_statistics(lab_t, shape, n_class, [gate], stream=stream, counts=counts)['qc']


def device_gate(lab_t, shape, seq_name, seg4, name, n_class, stream=0, counts=None):
    """(passed, message) of the reference's gate for this sequence (qc_gates.gate_from_stats) from a uint8 label volume on the
    device; only the few hundred bytes of statistics cross to the host."""
    from .qc_gates import gate_from_stats
    return gate_from_stats(device_gate_stats(lab_t, shape, seq_name, seg4, n_class, stream, counts), seq_name, seg4, name)


def device_atrial_stats(lab_t, shape, n_class, affine, long_axis, stream=0):
    """atrial.frame_stats_host of the (X,Y,1,T) uint8 label volume ``lab_t`` (NIfTI order) on the device."""
    return label_statistics(lab_t, shape, n_class, [AtrialStats()], {'atrial': (affine, long_axis)}, stream)['atrial']


def aortic_sequence_device(image, engine, batch_slices=128, window=None, return_aux=False, qc=False, prob=False, confidence=False):
    """pipeline.aortic_prob_sequence (``window`` None: the frame-wise 'UNet' model in chunks of ``batch_slices``) or
    pipeline.aortic_lstm_prob_sequence (``window`` = (weight_R, weight_r, time_step): the windowed models, one cine per slice
    position) + the argmax of deploy_network_ao.py:189 with the array work on the GPU: (X,Y,Z,T) float32 / uint8 / int16 / uint16
    aortic cine -> int32 label volume (X,Y,Z,T), the default --z_score pre-processing.  Only the raw volume goes in and uint8
    labels come back (the host path moves the padded float32 cine in and 3 float32 probability maps per voxel out, and spends more
    time in np.percentile / np.argmax than the network takes); the frame-wise engine's label map IS the lowest-index argmax of the
    float32 probabilities it would return (``softmax_argmax``, csrc/kernels.h).  With ``return_aux``: the z-score statistics and
    ``aux['counts']`` = pixels of each class per frame (what eval_aortic_area.py:60-78 turns into areas); with ``qc``,
    ``aux['qc']`` = device_qc_stats of the cine and the labels, the input of aorta_qc.aorta_qc_full; with ``prob`` (windowed
    forward only: 78 MB for 100 frames), ``aux['prob']`` (X,Y,Z,T,C); with ``confidence``, ``aux['confidence']`` = confidence.cells_host of
    the probabilities (ConfidenceStats: the windowed forward's averaged probabilities as they lie on the device, the frame-wise forward's
    chunk by chunk)."""
    import torch
    host = 'pipeline.aortic_prob_sequence' if window is None else 'pipeline.aortic_lstm_prob_sequence'
    if (qc or prob or confidence) and not return_aux:
        raise ValueError('qc=True, prob=True and confidence=True return their results in aux: pass return_aux')
    if prob and window is None:
        raise ValueError('prob=True: only the windowed forward leaves probabilities')
    if image.ndim != 4:
        raise TypeError('expected a 4-D (X,Y,Z,T) cine; use %s otherwise' % host)
    _check_dtype(image, host)
    X, Y, Z, T = image.shape
    dev = torch.device('cuda', engine.device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    vol = _to_device(image, dev)
    mu, den, n_roi, val_l = device_zscore_stats(vol, 10.0, stream, image.dtype)
    X2, Y2, x_pre, _, y_pre, _ = pad_amounts_fixed(X, Y)
    n_class = engine.arch.n_class
    batch = torch.empty((T, Z, X2, Y2), dtype=torch.float32, device=dev)
    zscore_pack(vol.data_ptr(), image.dtype, (X, Y, Z, T), vol.stride(), mu, den, (X2, Y2, x_pre, y_pre), batch.data_ptr(), stream)
    if window is not None:
        probs = torch.empty((T, Z, X2, Y2, n_class), dtype=torch.float32, device=dev)
    pred = torch.empty((T, Z, X2, Y2), dtype=torch.int32, device=dev)
    conf = ConfidenceStats(batch_slices, n_class, pad_amounts_fixed) if confidence else None
    per_chunk = chunk_statistics_buffers([conf] if conf else [], (X, Y, Z, T), n_class, dev) if window is None or conf is None else \
        [(conf, probs, torch.zeros(conf.sizes((X, Y, Z, T), n_class)[1], dtype=torch.int32, device=dev))]
    if window is None:
        forward_chunks(engine, batch.data_ptr(), pred.data_ptr(), T * Z, X2, Y2, batch_slices, stream,
                       [(stat, work.data_ptr(), out.data_ptr(), (X, Y, Z, T), (X2, Y2, x_pre, y_pre)) for stat, work, out in per_chunk])
    else:
        for z in range(Z):                                   # slice positions are independent cines (usually Z = 1)
            fr = batch[:, z] if Z == 1 else batch[:, z].contiguous()
            pr = probs[:, z] if Z == 1 else torch.empty((T, X2, Y2, n_class), dtype=torch.float32, device=dev)
            pd = pred[:, z] if Z == 1 else torch.empty((T, X2, Y2), dtype=torch.int32, device=dev)
            engine.run_cine_device(fr.data_ptr(), T, X2, Y2, pr.data_ptr(), pd.data_ptr(), *window, stream)
            if Z > 1:
                probs[:, z].copy_(pr)
                pred[:, z].copy_(pd)
        if conf is not None:                                 # the averaged probabilities of the whole cine lie on the device: one launch
            conf.launch_chunk(probs.data_ptr(), pred.data_ptr(), T * Z, 0, (X, Y, Z, T), (X2, Y2, x_pre, y_pre), n_class,
                              per_chunk[0][2].data_ptr(), stream)
    lab = torch.empty(X * Y * Z * T, dtype=torch.uint8, device=dev)
    counts = torch.empty((T, n_class), dtype=torch.int64, device=dev)
    _lib.check(_lib.lib.ukbb_fcn_unpack_labels(pred.data_ptr(), X, Y, Z, T, X2, Y2, x_pre, y_pre, n_class,
                                               lab.data_ptr(), counts.data_ptr(), stream), 'ukbb_fcn_unpack_labels')
    out = lab.cpu().numpy().reshape((X, Y, Z, T), order='F').astype(np.int32)
    if not return_aux:
        return out
    aux = {'mu': mu, 'den': den, 'n_roi': n_roi, 'val_l': val_l, 'counts': counts.cpu().numpy()}
    if qc:
        aux['qc'] = device_qc_stats(vol, lab, image.dtype, n_class, stream)
    if conf is not None:
        aux['confidence'] = conf.decode(per_chunk[0][2].cpu().numpy(), (X, Y, Z, T), n_class)
    if prob:
        aux['prob'] = probs[:, :, x_pre:x_pre + X, y_pre:y_pre + Y].permute(2, 3, 1, 0, 4).cpu().numpy()
    return out, aux
