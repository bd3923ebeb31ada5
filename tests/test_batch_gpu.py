"""Batches of captures with one plan (sp_render_batch / sp_plan_execute_batch, k_frames_batch) on the device: every item's reply is
byte for byte the reply of that item rendered alone."""
import numpy as np
import pytest

import goldenlib
import siggen
from __graft_entry__ import load_package
from oracle import pyoracle

pytestmark = pytest.mark.gpu

KEYS = ("rgba", "gauge_mins", "gauge_maxs", "gauge_amps", "c_hist", "cB_hist", "dBfs_min", "dBfs_max")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _lut(count=256):
    i = np.arange(count)
    lut = np.stack([(i * 5) & 255, (i * 11 + 3) & 255, (255 - i) & 255], axis=1).astype(np.uint8)
    lut[0] = 0
    lut[-1] = 255
    return lut


def _same(a, b, where):
    bad = []
    for k in KEYS:
        x, y = a[k], b[k]
        if isinstance(x, float):
            if not (x == y or (x != x and y != y)) or np.signbit(x) != np.signbit(y):
                bad.append("%s: %s %r != %r" % (where, k, x, y))
        elif not np.array_equal(np.asarray(x), np.asarray(y)):
            bad.append("%s: %s differs" % (where, k))
    return bad


def _capture(fmt, samples, seed):
    gen = {"kind": "trinoise", "seed": seed, "step": 7321 + seed, "gshift": 11, "amp": 0.5, "namp": 0.02}
    return siggen.generate(fmt, gen, samples)


def test_golden_worker_cases_as_items_of_mixed_batches(pkg, ctx, golden):
    """Every worker vector of the real reference (the ones the single-render tests use) rendered as one item of a batch, between two
    filler items of other lengths and widths: the item's reply equals the reference's."""
    bad, seen = [], 0
    for c in golden.spec["worker_cases"]:
        e = golden.expected[c["name"]]
        if "reply" not in e:
            continue
        data = golden.input(c)
        win, weight = pyoracle.window(c["window"], c["n"])
        lut = golden.lut(c)
        fid, sw = pkg.parse_format(c["format"])
        elem = pkg.binding.Library.get().L.sp_format_element_size(fid)
        noise = np.random.default_rng(c["n"] + seen)
        fill_a = noise.integers(0, 256, (3 * c["n"] * sw + 5) // elem * elem, dtype=np.uint8)
        fill_b = noise.integers(0, 256, 40 * c["n"] * sw // elem * elem, dtype=np.uint8)
        outs = ctx.render_batch(c["format"], [fill_a, data, fill_b], c["n"], win, 1.0 / weight, c["gain"], c["range"], lut,
                                [7, c["width"], 37], c["channelMode"], c["waterfall"])
        bad += goldenlib.check_reply(outs[1], e["reply"], c["name"] + ": ")
        seen += 1
    assert seen >= 10
    assert not bad, bad[:30]


def _random_items(rng, fmt, n, count):
    sw = {"cu4": 1, "cs4": 1, "cu8": 2, "cs8": 2, "cs12": 3, "cs16": 4, "cf32": 8, "cf64": 16}[fmt]
    datas, widths = [], []
    for k in range(count):
        kind = rng.integers(0, 4)
        if kind == 0:
            samples = int(rng.integers(1, 2 * n))                 # shorter than a frame or barely longer: out of bounds
        elif kind == 1:
            samples = int(rng.integers(n, 40 * n))
        else:
            samples = int(rng.integers(n, 8 * n))
        w = int(rng.choice([0, 1, 2, 3, 5, 17, 32, 33, 64, 100, 257]))
        if kind == 3:
            w = max(w, 2)
            samples = n + (w - 1) * int(rng.integers(n + 1, 3 * n))  # sparse: stride above n, every frame inside
        data = _capture(fmt, samples, int(rng.integers(1, 1 << 30)))
        elem = 8 if fmt == "cf64" else (4 if fmt == "cf32" else (2 if sw in (2, 4) else 1))
        data = data[: len(data) // elem * elem]
        datas.append(data)
        widths.append(w)
    return datas, widths


@pytest.mark.parametrize("fmt,n,ch,wf", [("cu8", 512, False, False), ("cs16", 1024, False, True), ("cf32", 256, True, False),
                                         ("cs12", 2048, False, False), ("cu4", 64, False, False), ("cf64", 128, False, True),
                                         ("cs8", 8192, True, False), ("cu8", 4096, False, False)])
def test_random_batches_equal_single_renders(pkg, ctx, fmt, n, ch, wf):
    rng = np.random.default_rng(n + len(fmt) * 7 + ch * 3 + wf)
    win, weight = pkg.window("hann", n)
    lut = _lut()
    count = int(rng.integers(1, 300 if n <= 1024 else 24))
    datas, widths = _random_items(rng, fmt, n, count)
    outs = ctx.render_batch(fmt, datas, n, win, 1.0 / weight, 3.0, 40.0, lut, widths, ch, wf)
    uploaded = ctx.last_upload_bytes()
    bad = []
    for k in range(count):
        want = ctx.render(fmt, datas[k], n, win, 1.0 / weight, 3.0, 40.0, lut, widths[k], ch, wf)
        bad += _same(outs[k], want, "item %d (w=%d, %d bytes)" % (k, widths[k], datas[k].size))
    assert not bad, bad[:20]
    assert uploaded == sum(d.size for d in datas)


def _device_batch(ctx, plan, datas, widths, n, lut_len, fill=0xA5, null_keys=()):
    """Uploads the captures, allocates every item's outputs with guard bytes around them (pre-filled with garbage), runs
    execute_batch and returns (outputs, guards intact)."""
    G = 64
    allocs, items, layout = [], [], []
    for d, w in zip(datas, widths):
        d_in = ctx.alloc(max(d.size, 16))
        allocs.append(d_in)
        if d.size:
            ctx.upload(d_in, d)
        sizes = {"rgba": 4 * w * n, "gauge_mins": w, "gauge_maxs": w, "gauge_amps": w, "c_hist": 8 * lut_len, "cb_hist": 8000,
                 "dbfs_minmax": 16}
        outs, lay = {}, {}
        for key, sz in sizes.items():
            if key in null_keys:
                continue
            buf = ctx.alloc(sz + 2 * G + 16)
            allocs.append(buf)
            ctx.memset(buf, fill, sz + 2 * G + 16)
            outs[key] = buf + G
            lay[key] = (buf, sz)
        items.append((d_in, d.size, w, outs))
        layout.append(lay)
    plan.execute_batch(items)
    ctx.synchronize()
    res, guards_ok = [], True
    for lay in layout:
        r = {}
        for key, (buf, sz) in lay.items():
            raw = ctx.download(buf, sz + 2 * G + 16)
            guards_ok &= bool(np.all(raw[:G] == fill) and np.all(raw[G + sz:] == fill))
            body = raw[G:G + sz]
            r[key] = body.view(np.uint64) if key in ("c_hist", "cb_hist") else (body.view(np.float64) if key == "dbfs_minmax" else body)
        res.append(r)
    for a in allocs:
        ctx.free(a)
    return res, guards_ok


def test_device_batch_overwrites_garbage_keeps_guards_and_skips_null_outputs(pkg, ctx):
    n, fmt = 512, "cu8"
    win, weight = pkg.window("blackmanHarris", n)
    lut = _lut()
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
    rng = np.random.default_rng(5)
    datas, widths = _random_items(rng, fmt, n, 40)
    for null_keys in ((), ("rgba", "gauge_amps"), ("c_hist", "dbfs_minmax", "gauge_mins")):
        res, guards = _device_batch(ctx, plan, datas, widths, n, len(lut), null_keys=null_keys)
        assert guards, null_keys
        for k, (d, w) in enumerate(zip(datas, widths)):
            want = ctx.render(fmt, d, n, win, 1.0 / weight, 6.0, 30.0, lut, w)
            r = res[k]
            for key, wk in (("rgba", "rgba"), ("gauge_mins", "gauge_mins"), ("gauge_maxs", "gauge_maxs"), ("gauge_amps", "gauge_amps"),
                            ("c_hist", "c_hist"), ("cb_hist", "cB_hist")):
                if key in r:
                    assert np.array_equal(r[key], want[wk]), (k, key, null_keys)
            if "dbfs_minmax" in r:
                assert r["dbfs_minmax"].tobytes() == np.array([want["dBfs_min"], want["dBfs_max"]]).tobytes(), (k, null_keys)
    plan.close()


def test_single_renders_and_batches_interleave_on_one_context(pkg, ctx):
    """single render -> batch -> single render -> execute_from_host -> batch, nothing synchronised in between by the caller."""
    n, fmt = 1024, "cs16"
    win, weight = pkg.window("hann", n)
    lut = _lut()
    rng = np.random.default_rng(11)
    datas, widths = _random_items(rng, fmt, n, 12)
    want = [ctx.render(fmt, d, n, win, 1.0 / weight, 0.0, 50.0, lut, w) for d, w in zip(datas, widths)]
    one = _capture(fmt, 300 * n, 99)
    one_want = ctx.render(fmt, one, n, win, 1.0 / weight, 0.0, 50.0, lut, 640)
    a = ctx.render(fmt, one, n, win, 1.0 / weight, 0.0, 50.0, lut, 640)
    b = ctx.render_batch(fmt, datas, n, win, 1.0 / weight, 0.0, 50.0, lut, widths)
    c = ctx.render(fmt, one, n, win, 1.0 / weight, 0.0, 50.0, lut, 640)
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 0.0, 50.0, lut)
    d_img = ctx.alloc(4 * 640 * n)
    keep = plan.execute_from_host(one, 640, rgba=d_img)
    d = ctx.render_batch(fmt, datas, n, win, 1.0 / weight, 0.0, 50.0, lut, widths)
    ctx.synchronize()
    img = ctx.download(d_img, 4 * 640 * n)
    del keep
    ctx.free(d_img)
    plan.close()
    bad = _same(a, one_want, "single 1") + _same(c, one_want, "single 2")
    for k in range(len(datas)):
        bad += _same(b[k], want[k], "batch 1 item %d" % k) + _same(d[k], want[k], "batch 2 item %d" % k)
    assert np.array_equal(img, one_want["rgba"])
    assert not bad, bad[:20]


@pytest.mark.parametrize("n", [16384, 32])
def test_plans_outside_the_frame_loop_render_item_by_item(pkg, ctx, n):
    fmt = "cu8"
    win, weight = pkg.window("hamming", n)
    lut = _lut()
    rng = np.random.default_rng(n)
    datas, widths = _random_items(rng, fmt, n, 5)
    widths = [min(w, 40) for w in widths]
    outs = ctx.render_batch(fmt, datas, n, win, 1.0 / weight, 0.0, 60.0, lut, widths)
    bad = []
    for k in range(len(datas)):
        bad += _same(outs[k], ctx.render(fmt, datas[k], n, win, 1.0 / weight, 0.0, 60.0, lut, widths[k]), "item %d" % k)
    assert not bad, bad[:20]


def test_large_batch_of_config1_items(pkg, ctx):
    """1 024 config-1 items (cu8, n = 512, 2^20 samples, width 2 048) from the device synthesiser in one sp_plan_execute_batch: 20 of
    them compared with the oracle (oracle/pyoracle.py, an independent restatement of lib/worker.js), the histogram totals of all of
    them checked."""
    n, fmt, W, S, K = 512, "cu8", 2048, 1 << 20, 1024
    win, weight = pkg.window("blackmanHarris", n)
    lut = _lut()
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 6.0, 30.0, lut)
    nbytes = 2 * S
    d_in = ctx.alloc(K * nbytes)
    gen = dict(seed=4242, step=7321, gshift=11, amp=0.5, namp=0.02)
    ctx.synth_trinoise(d_in, fmt, 0, K * S, gen["seed"], gen["step"], gen["gshift"], gen["amp"], gen["namp"])
    img_b, rec_b = 4 * W * n, 8 * (len(lut) + 1000) + 16
    d_img = ctx.alloc(K * img_b)
    d_rec = ctx.alloc(K * rec_b)
    items = []
    for k in range(K):
        r = d_rec + k * rec_b
        items.append((d_in + k * nbytes, nbytes, W, {"rgba": d_img + k * img_b, "c_hist": r, "cb_hist": r + 8 * len(lut),
                                                       "dbfs_minmax": r + 8 * (len(lut) + 1000)}))
    plan.execute_batch(items)
    ctx.synchronize()
    recs = ctx.download(d_rec, K * rec_b).reshape(K, rec_b)
    for k in range(K):
        c = recs[k, :8 * len(lut)].view(np.uint64)
        cb = recs[k, 8 * len(lut):8 * (len(lut) + 1000)].view(np.uint64)
        assert int(c.sum()) == W * n and int(cb.sum()) == W * n, k
    for k in np.linspace(0, K - 1, 20).astype(int):
        data = ctx.download(d_in + int(k) * nbytes, nbytes)
        want = pyoracle.render(fmt, data, n, win, 1.0 / weight, 6.0, 30.0, lut, W)
        assert np.array_equal(ctx.download(d_img + int(k) * img_b, img_b), want["rgba"]), k
        assert np.array_equal(recs[k, :8 * len(lut)].view(np.uint64).astype(np.int64), want["c_hist"]), k
        assert np.array_equal(recs[k, 8 * len(lut):8 * (len(lut) + 1000)].view(np.uint64).astype(np.int64), want["cB_hist"]), k
        mm = recs[k, 8 * (len(lut) + 1000):].view(np.float64)
        assert mm[0] == want["dBfs_min"] and mm[1] == want["dBfs_max"], k
    for a in (d_in, d_img, d_rec):
        ctx.free(a)
    plan.close()


def test_device_queued_single_and_batch_launches_interleave_without_syncs(pkg, ctx):
    """sp_plan_execute -> sp_plan_execute_batch -> sp_plan_execute -> sp_plan_execute_batch queued back to back on one stream, nothing
    synchronised in between: every reply is right (the batch has no request number; the single requests keep theirs)."""
    n, fmt, W = 256, "cu8", 300
    win, weight = pkg.window("hann", n)
    lut = _lut()
    plan = ctx.plan(fmt, n, win, 1.0 / weight, 0.0, 45.0, lut)
    rng = np.random.default_rng(21)
    datas, widths = _random_items(rng, fmt, n, 9)
    single = _capture(fmt, 120 * n, 77)
    want_single = ctx.render(fmt, single, n, win, 1.0 / weight, 0.0, 45.0, lut, W)
    want = [ctx.render(fmt, d, n, win, 1.0 / weight, 0.0, 45.0, lut, w) for d, w in zip(datas, widths)]
    allocs = []

    def dalloc(nb):
        p = ctx.alloc(max(nb, 16))
        allocs.append(p)
        return p
    d_single = dalloc(single.size)
    ctx.upload(d_single, single)
    d_caps = []
    for d in datas:
        p = dalloc(d.size)
        if d.size:
            ctx.upload(p, d)
        d_caps.append(p)
    ctx.synchronize()

    def single_outs():
        return {"rgba": dalloc(4 * W * n), "c_hist": dalloc(8 * len(lut)), "cb_hist": dalloc(8000), "dbfs_minmax": dalloc(16)}

    def batch_outs():
        return [{"rgba": dalloc(4 * w * n), "c_hist": dalloc(8 * len(lut)), "cb_hist": dalloc(8000), "dbfs_minmax": dalloc(16),
                 "gauge_mins": dalloc(w)} for w in widths]
    s1, b1, s2, b2 = single_outs(), batch_outs(), single_outs(), batch_outs()
    plan.execute(d_single, single.size, W, **s1)
    plan.execute_batch([(p, d.size, w, o) for p, d, w, o in zip(d_caps, datas, widths, b1)])
    plan.execute(d_single, single.size, W, **s2)
    plan.execute_batch([(p, d.size, w, o) for p, d, w, o in zip(d_caps, datas, widths, b2)])
    ctx.synchronize()
    bad = []
    for tag, o in (("single 1", s1), ("single 2", s2)):
        if not np.array_equal(ctx.download(o["rgba"], 4 * W * n), want_single["rgba"]) \
                or not np.array_equal(ctx.download(o["cb_hist"], 8000, np.uint64), want_single["cB_hist"]):
            bad.append(tag)
    for tag, outs in (("batch 1", b1), ("batch 2", b2)):
        for k, (o, w) in enumerate(zip(outs, widths)):
            ok = np.array_equal(ctx.download(o["rgba"], 4 * w * n), want[k]["rgba"])
            ok &= np.array_equal(ctx.download(o["c_hist"], 8 * len(lut), np.uint64), want[k]["c_hist"])
            ok &= np.array_equal(ctx.download(o["gauge_mins"], w), want[k]["gauge_mins"])
            mm = ctx.download(o["dbfs_minmax"], 16, np.float64)
            ok &= mm.tobytes() == np.array([want[k]["dBfs_min"], want[k]["dBfs_max"]]).tobytes()
            if not ok:
                bad.append("%s item %d" % (tag, k))
    for p in allocs:
        ctx.free(p)
    plan.close()
    assert not bad, bad
