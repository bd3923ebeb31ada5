"""The numeric spectrogram, its exact mean, its exact variance sums, its exact lagged covariances, its exact block means and their colouring, its exact band sums, its exact spectral moments, its peak track, its occupancy counts, its percentile traces and its
burst lists as torch tensors: sp_plan_execute_power / _mean / _variance / _lagcov / _blockmean / _bandpower / _moments / _track / _occupancy / _quantile / _bursts on torch's current
stream.

`power(plan, capture, width)` hands a detector, a model or a viewer the f64 plane |X|^2 [width, n] behind every other reply of the
library (include/spectroplot_hip.h, "Power plane replies"), resident on the capture's device and ordered on torch's current stream:
whatever the caller queues next on that stream - a reduction, a percentile, a network - sees the finished plane without a host
synchronisation.
"""
import contextlib

import torch

from . import binding


def _check_capture(name, capture):
    if capture.dtype != torch.uint8 or not capture.is_cuda or not capture.is_contiguous():
        raise binding.SpectroplotError(binding.SP_ERR_INVALID_ARG, "tensor.%s: capture must be a contiguous uint8 CUDA tensor" % name)


@contextlib.contextmanager
def _on_current_stream(ctx, dev, operands):
    """Binds the context to torch's current stream of `dev` for the calls in the body (see power()), records the operands on it and puts
    the context's previous binding back on the way out."""
    current = torch.cuda.current_stream(dev)
    stream = current
    if stream.cuda_stream == 0:
        stream = torch.cuda.Stream(device=dev)
        stream.wait_stream(current)   # whatever produced the capture there
    previous = ctx.get_stream()
    if previous != stream.cuda_stream:
        ctx.synchronize()
    ctx.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            for t in operands:
                t.record_stream(stream)
            yield
    finally:
        ctx.set_stream(previous)
    if stream is not current:
        current.wait_stream(stream)   # the caller's stream (the null stream) sees the result in order


def power(plan, capture, width, db=False, out=None):
    """|X|^2 of every frame and bin of `capture` (a uint8 CUDA tensor: the raw bytes) as a float64 tensor [width, n] on the same device,
    row y of frame x at [x, y] (image row order, lib/worker.js:90); db=True converts it in place to the dB plane with the plan's
    block_norm and gain.  `plan` is a binding.Plan of the sample detector on that device.  `out`: a contiguous float64 tensor of
    width * n elements on the device to write into (returned reshaped), else a new one.

    The launch is queued on torch's current stream, bound to the plan's context as sharding.render_sharded_device binds it: an
    explicit stream where the current one is the null stream (its handle, 0, means "your own stream" to the context), the operands
    recorded on it, and the context's previous binding put back on the way out.  The call does not wait for the plane: only where the
    context was bound to another stream is that stream's earlier work drained first (the context's workspaces rely on one stream's
    order)."""
    _check_capture("power", capture)
    ctx, n = plan.ctx, plan.n
    dev = capture.device
    width = int(width)
    count = max(width, 0) * n
    if out is None:
        out = torch.empty((max(width, 0), n), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or out.device != dev or not out.is_contiguous() or out.numel() != count:
        raise binding.SpectroplotError(binding.SP_ERR_INVALID_ARG, "tensor.power: out must be a contiguous float64 tensor of width * n on the capture's device")
    with _on_current_stream(ctx, dev, (capture, out)):
        plan.execute_power(capture.data_ptr(), capture.numel(), width, out.data_ptr())
        if db and count:
            plan.power_to_db(out.data_ptr(), count, out.data_ptr())
    return out.view(max(width, 0), n)


def mean(plan, capture, width):
    """The exact mean-power trace of `capture` (a uint8 CUDA tensor: the raw bytes) as a float64 tensor [n] on the same device: the
    correctly rounded sum of |X|^2 over the `width` frames divided by width, per image row (include/spectroplot_hip.h, "Exact
    mean-power trace").  `plan` is a binding.Plan of the sample detector on that device.  Queued on torch's current stream exactly as
    power() queues its plane; the plane itself is never held whole."""
    _check_capture("mean", capture)
    out = torch.empty((plan.n,), dtype=torch.float64, device=capture.device)
    with _on_current_stream(plan.ctx, capture.device, (capture, out)):
        plan.execute_mean(capture.data_ptr(), capture.numel(), int(width), out.data_ptr())
    return out


def variance(plan, capture, width):
    """The exact variance sums of `capture` (a uint8 CUDA tensor: the raw bytes) as a float64 tensor [3, n] on the same device: per
    image row the correctly rounded sum of |X|^2 over the `width` frames, the correctly rounded sum of its exact squares, and the
    correctly rounded width * sum of squares - sum**2, the subtraction done exactly (include/spectroplot_hip.h, "Exact variance and
    spectral-kurtosis traces").  out[0] / width is mean()'s trace bit for bit; the variance is out[2] / width**2 and the spectral
    kurtosis (width + 1) / (width - 1) * out[2] / out[0]**2, tensor operations on the same stream without a cancellation.  `plan` is a
    binding.Plan of the sample detector on that device.  Queued on torch's current stream exactly as power() queues its plane; the
    plane itself is never held whole."""
    _check_capture("variance", capture)
    out = torch.empty((3, plan.n), dtype=torch.float64, device=capture.device)
    with _on_current_stream(plan.ctx, capture.device, (capture, out)):
        plan.execute_variance(capture.data_ptr(), capture.numel(), int(width), out.data_ptr())
    return out


def lagcov(plan, capture, width, bands, pairs, lags):
    """The exact lagged covariance sums of `capture` (a uint8 CUDA tensor: the raw bytes) as a float64 tensor [3, npairs, lags] on the
    same device: per pair (ia, ib) of the bands (y0, y1) of image rows and per lag l, over the N = width - lags + 1 terms every lag
    has, the correctly rounded sum of a[x] * b[x + l], the correctly rounded N * that sum - sum(a) * sum(b's window) - signed, the
    subtraction done exactly - and the correctly rounded sum of b's window, a and b the band-power series bandpower() gives
    (include/spectroplot_hip.h, "Exact lagged covariances").  The covariance at lag l is out[1] / N**2 and the correlation coefficient
    binding.lag_correlation's form, tensor operations on the same stream.  `plan` is a binding.Plan of the sample detector on that
    device.  Queued on torch's current stream exactly as power() queues its plane; the plane itself is never held whole."""
    _check_capture("lagcov", capture)
    bands = [(int(y0), int(y1)) for y0, y1 in bands]
    pairs = [(int(i), int(j)) for i, j in pairs]
    out = torch.empty((3, len(pairs), max(int(lags), 0)), dtype=torch.float64, device=capture.device)
    with _on_current_stream(plan.ctx, capture.device, (capture, out)):
        plan.execute_lagcov(capture.data_ptr(), capture.numel(), int(width), bands, pairs, int(lags), out.data_ptr() if out.numel() else 0)
    return out


def blockmean(plan, capture, width, group):
    """The averaged spectrogram of `capture` (a uint8 CUDA tensor: the raw bytes) as a float64 tensor [columns, n] on the same device:
    per column of `group` frames and per image row the correctly rounded sum of |X|^2 over the column's frames divided by their number
    (include/spectroplot_hip.h, "Averaged spectrogram"); columns = ceil(width / group).  The result is itself a frame-major power plane.
    `plan` is a binding.Plan of the sample detector on that device.  Queued on torch's current stream exactly as power() queues its
    plane; the plane itself is never held whole."""
    _check_capture("blockmean", capture)
    columns = binding.blockmean_columns(width, group)
    out = torch.empty((columns, plan.n), dtype=torch.float64, device=capture.device)
    with _on_current_stream(plan.ctx, capture.device, (capture, out)):
        plan.execute_blockmean(capture.data_ptr(), capture.numel(), int(width), int(group), out.data_ptr() if out.numel() else 0)
    return out


def power_to_index(plan, plane):
    """The colour-index image of `plane` (a contiguous float64 CUDA tensor [width, n]: a power plane, a block-mean plane) as a uint8
    tensor on the same device, coloured with the plan's gain, range and LUT length exactly as the frame loop colours its own pixels
    (include/spectroplot_hip.h, sp_plan_power_to_index): [n, width] for a spectrogram plan, [width, n] for a waterfall plan.  Queued on
    torch's current stream exactly as power() queues its plane."""
    if plane.dtype != torch.float64 or not plane.is_cuda or not plane.is_contiguous() or plane.dim() != 2 or plane.shape[1] != plan.n:
        raise binding.SpectroplotError(binding.SP_ERR_INVALID_ARG, "tensor.power_to_index: plane must be a contiguous float64 CUDA tensor [width, n]")
    width = plane.shape[0]
    out = torch.empty((width, plan.n) if plan.waterfall else (plan.n, width), dtype=torch.uint8, device=plane.device)
    with _on_current_stream(plan.ctx, plane.device, (plane, out)):
        plan.power_to_index(plane.data_ptr(), width, out.data_ptr() if out.numel() else 0)
    return out


def bandpower(plan, capture, width, bands):
    """The exact band-power series of `capture` (a uint8 CUDA tensor: the raw bytes) as a float64 tensor [count, width] on the same
    device: per band (y0, y1) of image rows - a half-open range - and per frame the correctly rounded sum of |X|^2 over the band's
    rows (include/spectroplot_hip.h, "Exact band-power series"; binding.band_rows turns a frequency range into rows).  `plan` is a
    binding.Plan of the sample detector on that device.  Queued on torch's current stream exactly as power() queues its plane; the
    plane itself is never held whole."""
    _check_capture("bandpower", capture)
    bands = [(int(y0), int(y1)) for y0, y1 in bands]
    out = torch.empty((len(bands), max(int(width), 0)), dtype=torch.float64, device=capture.device)
    with _on_current_stream(plan.ctx, capture.device, (capture, out)):
        plan.execute_bandpower(capture.data_ptr(), capture.numel(), int(width), bands, out.data_ptr())
    return out


def moments(plan, capture, width, bands, order=1):
    """The exact spectral moments of `capture` (a uint8 CUDA tensor: the raw bytes) as a float64 tensor [order + 1, count, width] on
    the same device: per band (y0, y1) of image rows - a half-open range - and per frame the correctly rounded sums of
    (y - y0)**k * |X|^2 over the band's rows, k = 0 .. order (include/spectroplot_hip.h, "Exact spectral moments").  out[0] is
    bandpower()'s series bit for bit; the centroid row is y0 + out[1] / out[0] and the RMS width in rows
    sqrt(out[2] / out[0] - (out[1] / out[0])**2), one or two tensor operations each on the same stream.  `plan` is a binding.Plan of
    the sample detector on that device.  Queued on torch's current stream exactly as power() queues its plane; the plane itself is
    never held whole."""
    _check_capture("moments", capture)
    bands = [(int(y0), int(y1)) for y0, y1 in bands]
    out = torch.empty((max(int(order), 0) + 1, len(bands), max(int(width), 0)), dtype=torch.float64, device=capture.device)
    with _on_current_stream(plan.ctx, capture.device, (capture, out)):
        plan.execute_moments(capture.data_ptr(), capture.numel(), int(width), bands, int(order), out.data_ptr())
    return out


def track(plan, capture, width, bands):
    """The peak track of `capture` (a uint8 CUDA tensor: the raw bytes) as an int32 tensor [count, width] and a float64 tensor
    [count, width] on the same device: per band (y0, y1) of image rows - a half-open range - and per frame the strongest row that is
    not a NaN (the smallest among equal ones, -1 where there is none) and its |X|^2 bit for bit (NaN where there is none)
    (include/spectroplot_hip.h, "Peak track"; binding.row_freq turns a row into a frequency).  `plan` is a binding.Plan of the sample
    detector on that device.  Queued on torch's current stream exactly as power() queues its plane; the plane itself is never held
    whole."""
    _check_capture("track", capture)
    bands = [(int(y0), int(y1)) for y0, y1 in bands]
    shape = (len(bands), max(int(width), 0))
    rows = torch.empty(shape, dtype=torch.int32, device=capture.device)
    peaks = torch.empty(shape, dtype=torch.float64, device=capture.device)
    with _on_current_stream(plan.ctx, capture.device, (capture, rows, peaks)):
        plan.execute_track(capture.data_ptr(), capture.numel(), int(width), bands, rows.data_ptr(), peaks.data_ptr())
    return rows, peaks


def occupancy(plan, capture, width, threshold, bands=()):
    """The occupancy counts of `capture` (a uint8 CUDA tensor: the raw bytes) as two int32 tensors on the same device, rows [n] and
    frames [count, width]: rows[y] is the number of frames whose |X|^2 at image row y is >= threshold[y], frames[b, x] the number of rows
    of band (y0, y1) - a half-open range of image rows - that reach theirs in frame x; a NaN on either side is no hit
    (include/spectroplot_hip.h, "Occupancy counts").  The library's words are uint32; no count reaches 2^31, so they are int32 here.
    threshold: a Python float, for every row, or a contiguous float64 tensor of n values on the capture's device.  `plan` is a
    binding.Plan of the sample detector on that device.  Queued on torch's current stream exactly as power() queues its plane; the plane
    itself is never held whole."""
    _check_capture("occupancy", capture)
    dev, n = capture.device, plan.n
    if isinstance(threshold, torch.Tensor):
        if threshold.dtype != torch.float64 or threshold.device != dev or not threshold.is_contiguous() or threshold.numel() != n:
            raise binding.SpectroplotError(binding.SP_ERR_INVALID_ARG,
                                           "tensor.occupancy: threshold must be a number or a contiguous float64 tensor of n on the capture's device")
    else:
        threshold = torch.full((n,), float(threshold), dtype=torch.float64, device=dev)
    bands = [(int(y0), int(y1)) for y0, y1 in bands]
    rows = torch.empty((n,), dtype=torch.int32, device=dev)
    frames = torch.empty((len(bands), max(int(width), 0)), dtype=torch.int32, device=dev)
    with _on_current_stream(plan.ctx, dev, (capture, threshold, rows, frames)):
        plan.execute_occupancy(capture.data_ptr(), capture.numel(), int(width), threshold.data_ptr(), bands, rows.data_ptr(),
                               frames.data_ptr() if frames.numel() else 0)
    return rows, frames


def quantile(plan, capture, width, ranks):
    """The percentile traces of `capture` (a uint8 CUDA tensor: the raw bytes) as a float64 tensor [count, n] on the same device: per
    rank k of `ranks` and image row y element k of the row's `width` values of |X|^2 sorted ascending - np.sort(plane[:, y])[k] bit for
    bit, every NaN behind +inf (include/spectroplot_hip.h, "Percentile traces").  A quantile q becomes a rank through
    binding.quantile_rank(width, q) (numpy's method='lower').  `plan` is a binding.Plan of the sample detector on that device.  Queued
    on torch's current stream exactly as power() queues its plane; the context keeps the plane as keys, 8 * n * width bytes."""
    _check_capture("quantile", capture)
    ranks = [int(k) for k in ranks]
    out = torch.empty((len(ranks), plan.n), dtype=torch.float64, device=capture.device)
    with _on_current_stream(plan.ctx, capture.device, (capture, out)):
        plan.execute_quantile(capture.data_ptr(), capture.numel(), int(width), ranks, out.data_ptr() if out.numel() else 0)
    return out


def bursts(plan, capture, width, bands, hi, lo, max_bursts):
    """The burst lists of `capture` (a uint8 CUDA tensor: the raw bytes) as two int32 tensors on the same device, counts [count] and
    edges [count, max_bursts, 2]: per band (y0, y1) of image rows a Schmitt trigger along the frames of its exact band sum - ON from a
    frame with sum >= hi, OFF from one with sum < lo, OFF in front of frame 0 - the total number of its bursts and start and end of the
    first max_bursts of them, -1 behind those (include/spectroplot_hip.h, "Burst lists").  The library's counts are uint32; none
    reaches 2^31, so they are int32 here.  hi, lo: a Python float for every band, or `count` of them.  `plan` is a binding.Plan of the
    sample detector on that device.  Queued on torch's current stream exactly as power() queues its plane."""
    _check_capture("bursts", capture)
    bands = [(int(y0), int(y1)) for y0, y1 in bands]
    m = max(int(max_bursts), 0)
    counts = torch.empty((len(bands),), dtype=torch.int32, device=capture.device)
    edges = torch.empty((len(bands), m, 2), dtype=torch.int32, device=capture.device)
    with _on_current_stream(plan.ctx, capture.device, (capture, counts, edges)):
        plan.execute_bursts(capture.data_ptr(), capture.numel(), int(width), bands, hi, lo, int(max_bursts),
                            counts.data_ptr() if counts.numel() else 0, edges.data_ptr() if edges.numel() else 0)
    return counts, edges


def pulses(plan, capture, width, bands, hi, lo, max_bursts):
    """The burst lists of `capture` as bursts() gives them and the measurements of every listed burst, five tensors on the capture's
    device: counts int32 [count], edges int32 [count, max_bursts, 2], energy float64 [count, max_bursts], peak float64 [count,
    max_bursts] and peak_at int32 [count, max_bursts].  energy is the exact sum of the burst's frames of the band sum rounded once
    (math.fsum), peak the largest of them and peak_at the earliest frame that holds it; behind the listed bursts -1 and the all-ones
    NaN (include/spectroplot_hip.h, "Burst measurements").  Queued on torch's current stream exactly as bursts() queues its lists."""
    _check_capture("pulses", capture)
    bands = [(int(y0), int(y1)) for y0, y1 in bands]
    m = max(int(max_bursts), 0)
    dev = capture.device
    counts = torch.empty((len(bands),), dtype=torch.int32, device=dev)
    edges = torch.empty((len(bands), m, 2), dtype=torch.int32, device=dev)
    energy = torch.empty((len(bands), m), dtype=torch.float64, device=dev)
    peak = torch.empty((len(bands), m), dtype=torch.float64, device=dev)
    peak_at = torch.empty((len(bands), m), dtype=torch.int32, device=dev)
    some = edges.numel() > 0
    with _on_current_stream(plan.ctx, dev, (capture, counts, edges, energy, peak, peak_at)):
        plan.execute_pulses(capture.data_ptr(), capture.numel(), int(width), bands, hi, lo, int(max_bursts),
                            counts.data_ptr() if counts.numel() else 0, edges.data_ptr() if some else 0, energy.data_ptr() if some else 0,
                            peak.data_ptr() if some else 0, peak_at.data_ptr() if some else 0)
    return counts, edges, energy, peak, peak_at
