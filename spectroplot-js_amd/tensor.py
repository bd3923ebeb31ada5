"""The numeric spectrogram as a torch tensor: sp_plan_execute_power on torch's current stream.

`power(plan, capture, width)` hands a detector, a model or a viewer the f64 plane |X|^2 [width, n] behind every other reply of the
library (include/spectroplot_hip.h, "Power plane replies"), resident on the capture's device and ordered on torch's current stream:
whatever the caller queues next on that stream - a reduction, a percentile, a network - sees the finished plane without a host
synchronisation.
"""
import torch

from . import binding


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
    if capture.dtype != torch.uint8 or not capture.is_cuda or not capture.is_contiguous():
        raise binding.SpectroplotError(binding.SP_ERR_INVALID_ARG, "tensor.power: capture must be a contiguous uint8 CUDA tensor")
    ctx, n = plan.ctx, plan.n
    dev = capture.device
    width = int(width)
    count = max(width, 0) * n
    if out is None:
        out = torch.empty((max(width, 0), n), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or out.device != dev or not out.is_contiguous() or out.numel() != count:
        raise binding.SpectroplotError(binding.SP_ERR_INVALID_ARG, "tensor.power: out must be a contiguous float64 tensor of width * n on the capture's device")
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
            capture.record_stream(stream)
            out.record_stream(stream)
            plan.execute_power(capture.data_ptr(), capture.numel(), width, out.data_ptr())
            if db and count:
                plan.power_to_db(out.data_ptr(), count, out.data_ptr())
    finally:
        ctx.set_stream(previous)
    if stream is not current:
        current.wait_stream(stream)   # the caller's stream (the null stream) sees the plane in order
    return out.view(max(width, 0), n)
