'use strict'
/**
 * HipWorker — a Worker-shaped object for triq-org/spectroplot-js' `workerOrUrl` option, backed by the MI355X HIP library.
 *
 * The reference constructs its render workers with `new workerOrUrl()` when the option is not a URL string
 * (lib/spectroplot.js:100-116) and only uses two members: `postMessage(message, transfer)` and an assignable
 * `onmessage`.  This class provides exactly that, with the reference worker's contract:
 *   - a message without a `buffer` is ignored (the transferable probe, lib/worker.js:158-163, lib/spectroplot.js:118-119);
 *   - every render request produces exactly one reply, replies come back in request order (FIFO per instance);
 *   - the reply has the reference's fields (lib/worker.js:140-155): cB_hist, c_hist, dBfs_min, dBfs_max, offset,
 *     gauge_mins / gauge_maxs / gauge_amps (Uint8ClampedArray) and imageData.data (Uint8ClampedArray).
 * Where the reference worker would throw (and leave the caller's promise pending forever), this class reports an
 * `onerror({message, status})` event (or an 'error' listener) and still never emits a malformed reply.
 *
 * Instances are spread over the visible GPUs round-robin, so the reference's pool of N workers maps onto N devices
 * (its per-worker time slices become per-GPU shards).  There is no CPU fallback.
 */
const path = require('path')

let native = null
function addon() {
    if (!native) native = require(path.join(__dirname, '..', 'lib', 'spectroplot_hip.node'))
    return native
}

let nextDevice = 0

// Renders run on libuv's thread pool (4 threads unless UV_THREADPOOL_SIZE says otherwise, shared with fs / dns work), one thread
// per render in flight: a pool of N HipWorkers on N GPUs needs N of them.  The size is read when the pool first starts, so it is
// raised here, at load time, if nothing has been set; applications that have already used the pool must set it themselves.
function reserveThreads(devices) {
    const want = devices + 4
    const have = parseInt(process.env.UV_THREADPOOL_SIZE || '0', 10)
    if (!(have >= want)) process.env.UV_THREADPOOL_SIZE = String(Math.min(want, 1024))
}

/** cmap entries -> packed Uint8Array with the store semantics of the reference's Uint8ClampedArray image (worker.js:118-121). */
function packLut(cmap) {
    const lut = new Uint8ClampedArray(cmap.length * 3)
    for (let i = 0; i < cmap.length; i++) {
        lut[3 * i] = cmap[i][0]; lut[3 * i + 1] = cmap[i][1]; lut[3 * i + 2] = cmap[i][2]
    }
    return new Uint8Array(lut.buffer)
}

/** Float64Array -> Array of numbers, as the reference's reply carries its histograms (a loop: Array.from() on the two typed arrays took 46 us of a 270 us config-1 message, the loops take 6). */
function plainArray(t) {
    const a = new Array(t.length)
    for (let i = 0; i < t.length; i++) a[i] = t[i]
    return a
}

/**
 * `detector` of a message or named request -> enum sp_detector: absent / 'sample' = the reference (a column shows one frame), 'peak' =
 * max hold over the sub-frames up to the next column.  Anything else is an error (status -1), never a different image.
 */
function detectorId(d) {
    if (d === undefined || d === null || d === 'sample') return 0
    if (d === 'peak') return 1
    throw Object.assign(new Error(`detector must be 'sample' or 'peak', not ${JSON.stringify(d) || String(d)}`), { status: -1 })
}

/** `buffer` of a message as the addon reads it: the bytes of a typed-array view copied out into an ArrayBuffer, anything else as it is. */
function arrayBufferOf(buffer) {
    return ArrayBuffer.isView(buffer) ? buffer.buffer.slice(buffer.byteOffset, buffer.byteOffset + buffer.byteLength) : buffer
}

const refusal = (message, status) => Object.assign(new Error(message), { status })

// what `onerror` reports as the status of a rejected request (_queued): the error's own, or -1 where it has none
const ownStatus = err => err.status
const statusOrInvalid = err => err.status === undefined ? -1 : err.status

class HipWorker {
    /** @param {{device?: number}} [options] — device index; default: round-robin over the visible GPUs. */
    constructor(options) {
        this.onmessage = null
        this.onerror = null
        this._listeners = { message: [], error: [] }
        this._queue = Promise.resolve()
        this._closed = false
        const n = addon().deviceCount()
        if (nextDevice === 0) reserveThreads(n)
        if (n < 1) throw Object.assign(new Error('no HIP device: spectroplot-hip has no CPU fallback'), { status: -5 })
        this.device = options && options.device !== undefined ? options.device : (nextDevice++ % n)
        this._ctx = addon().createContext(this.device)
    }

    addEventListener(type, fn) { if (this._listeners[type]) this._listeners[type].push(fn) }
    removeEventListener(type, fn) {
        if (this._listeners[type]) this._listeners[type] = this._listeners[type].filter(f => f !== fn)
    }

    _emit(type, event) {
        const h = type === 'message' ? this.onmessage : this.onerror
        if (typeof h === 'function') h.call(this, event)
        for (const fn of this._listeners[type]) fn.call(this, event)
    }

    /** Same signature as Worker.postMessage; `transfer` is accepted and ignored (the buffer is read in place). */
    postMessage(message, transfer) { // eslint-disable-line no-unused-vars
        if (this._closed) return
        if (!(message && message.buffer)) return                        // worker.js:159
        // requests are serialised per instance, like one worker thread; the GPU work itself runs off the event loop
        // (a worker that has been terminated meanwhile neither starts queued requests nor reports anything)
        this._queue = this._queue.then(() => this._closed ? null : this._render(message)).then(
            reply => { if (reply && !this._closed) this._emit('message', { data: reply }) },
            err => { if (!this._closed) this._emit('error', { message: err.message, status: err.status, error: err }) })
    }

    _request(m) {
        const a = addon()
        const fmt = a.parseFormat(String(m.format))                     // upper-cases, aliases, unknown -> CU8
        const n = m.n
        // (the typed-array constructor converts an Array in one go; Float64Array.from() walks its iterator)
        const windowc = m.windowc instanceof Float64Array ? m.windowc : new Float64Array(m.windowc)
        return { format: fmt.id, buffer: arrayBufferOf(m.buffer), n, windowc, block_norm: m.block_norm, gain: m.gain, range: m.range,
            lut: packLut(m.cmap), width: m.width, channelMode: !!m.channelMode, waterfall: !!m.waterfall, detector: detectorId(m.detector) }
    }

    _wrap(m, r) {
        return {
            cB_hist: plainArray(r.cB_hist), c_hist: plainArray(r.c_hist), dBfs_min: r.dBfs_min, dBfs_max: r.dBfs_max,
            offset: m.offset,
            gauge_mins: new Uint8ClampedArray(r.gauge_mins), gauge_maxs: new Uint8ClampedArray(r.gauge_maxs),
            gauge_amps: new Uint8ClampedArray(r.gauge_amps), imageData: { data: new Uint8ClampedArray(r.rgba) },
        }
    }

    _render(m) {
        return new Promise((resolve, reject) => {
            let req
            try { req = this._request(m) } catch (e) { reject(e); return }
            // (Always on a libuv thread.  Rendering small requests on the calling thread was tried - the hand-off costs 0.06-0.08 ms of a
            // 0.36 ms config-1 message - and is slower: a chain of replies that resolves in microtasks never lets V8 run the finalisers
            // that return reply images to the pool, so every reply takes a fresh, unpinned block: 0.51 ms, tools/js_config1_message.js.)
            addon().render(this._ctx, req, (err, r) => err ? reject(err) : resolve(this._wrap(m, r)))
        })
    }

    /**
     * One request of the render* methods, in the instance's request order: `build()` makes the addon's request, `entry` names the
     * addon's function, `wrap(r)` turns its reply into what the promise resolves to.  A terminated worker, a refusal of the builder and
     * an error of the addon - thrown or called back - reject.  `report`: the status `onerror` is given for a rejection (ownStatus /
     * statusOrInvalid), or null for a method whose rejected promise is the only report.
     */
    _queued(build, entry, wrap, report) {
        const run = () => new Promise((resolve, reject) => {
            if (this._closed) { reject(new Error('worker has been terminated')); return }
            const req = build()                                         // (a throw in here is the promise's rejection)
            addon()[entry](this._ctx, req, (err, r) => err ? reject(err) : resolve(wrap(r)))
        })
        const p = this._queue.then(run)
        this._queue = p.then(() => null, err => {
            if (report && !this._closed) this._emit('error', { message: err.message, status: report(err), error: err })
        })
        return p
    }

    /**
     * A request by option names instead of evaluated arrays - not part of the reference worker's wire contract (its messages carry the
     * evaluated taper and colour map, lib/spectroplot.js:1213-1226), but what the reference's caller starts from: the library resolves
     * `window` and `cmap` with the reference's lookup rules and defaults (lib/utils.js:25-40, lib/spectroplot.js:238-264), evaluates
     * taper, block_norm and the end-forced colour map itself (:1113-1130) and keeps the device tables while names and numbers repeat.
     * @param {{buffer: ArrayBuffer, format: string, window: string, cmap: string, n: number, width: number, gain?: number,
     *          range?: number, channelMode?: boolean, waterfall?: boolean, offset?: number, detector?: 'sample'|'peak'}} o
     * @returns {Promise<object>} the reply, fields as in a worker reply; runs in the instance's request order
     */
    renderNamed(o) { return this._queued(() => this._namedRequest(o), 'renderNamed', r => this._wrap(o, r), null) }

    _namedRequest(o) {
        const buffer = arrayBufferOf(o.buffer)
        return { format: String(o.format), window: String(o.window === undefined ? '' : o.window), cmap: String(o.cmap === undefined ? '' : o.cmap),
            buffer, n: o.n, width: o.width, gain: o.gain === undefined ? 6 : o.gain, range: o.range === undefined ? 30 : o.range,
            channelMode: !!o.channelMode, waterfall: !!o.waterfall, detector: detectorId(o.detector) }
    }

    /**
     * Per-bin min-hold / max-hold traces of a request (sp_render_traces): the fields of a worker message - buffer, format, n, windowc,
     * block_norm, gain, range, width, channelMode; cmap, waterfall and offset are not looked at - in, two Float64Array(n) in image row
     * order out (row y of the spectrogram, column n - 1 - y of the waterfall).  No image is rendered.  Only the sample detector has
     * traces.  Runs in the instance's request order; a malformed field rejects (and reports `onerror`) and
     * never resolves to arrays.
     * @returns {Promise<{trace_min: Float64Array, trace_max: Float64Array}>}
     */
    renderTraces(m) {
        return this._queued(() => this._tracesRequest(m), 'renderTraces', r => ({ trace_min: r.trace_min, trace_max: r.trace_max }), ownStatus)
    }

    _tracesRequest(m) { return this._plainRequest(m, 'a traces request needs a buffer', 'traces of the peak detector are not supported') }

    /**
     * A request without a picture - no colour map, no `waterfall`, the sample detector only - with the kind's two refusal texts: of a
     * message without a buffer (status -1) and of the peak detector (status -4).  `own()` makes the kind's own fields, which follow the
     * shared ones; what it refuses is refused before anything is built.
     */
    _plainRequest(m, noBuffer, noPeak, own) {
        if (!(m && m.buffer)) throw refusal(noBuffer, -1)
        if (detectorId(m.detector) !== 0) throw refusal(noPeak, -4)
        const fields = own ? own() : null
        const fmt = addon().parseFormat(String(m.format))
        const windowc = m.windowc instanceof Float64Array ? m.windowc : new Float64Array(m.windowc)
        return Object.assign({ format: fmt.id, buffer: arrayBufferOf(m.buffer), n: m.n, windowc, block_norm: m.block_norm, gain: m.gain,
            range: m.range, width: m.width, channelMode: !!m.channelMode }, fields)
    }

    /** ... plus `db` of the options (renderPower, renderMean, renderBandPower, renderTrack), the kind's own fields behind it. */
    _dbRequest(m, opt, noBuffer, noPeak, own) {
        return this._plainRequest(m, noBuffer, noPeak, () => Object.assign({ db: !!(opt && opt.db) }, own && own()))
    }

    /**
     * The numeric spectrogram of a request (sp_render_power): the fields renderTraces reads in, |X|^2 of every frame and bin out as one
     * Float64Array(width * n), frame-major - frame x at power[x * n + y], y the image row (row y of the spectrogram, column n - 1 - y
     * of the waterfall) - or, with `{db: true}`, its dB plane (5 log10 |X|^2 + block_norm's dB, gain cancelled as the worker cancels
     * it).  No image is rendered; gain, range and colour map do not reach the power plane.  Only the sample detector has a plane.  Runs
     * in the instance's request order; a malformed field rejects (and reports `onerror`) and never resolves to an array.
     * @returns {Promise<{power: Float64Array, width: number, n: number}>}
     */
    renderPower(m, opt) {
        return this._queued(() => this._powerRequest(m, opt), 'renderPower', r => ({ power: r.power, width: r.width, n: r.n }), ownStatus)
    }

    _powerRequest(m, opt) {
        return this._dbRequest(m, opt, 'a power request needs a buffer', 'the power plane of the peak detector is not supported')
    }

    /** Synchronous form of renderPower (tests). */
    renderPowerSync(m, opt) { return addon().renderPowerSync(this._ctx, this._powerRequest(m, opt)) }

    /**
     * The exact mean-power trace of a request (sp_render_mean) - the average spectrum, a Welch PSD: the fields renderTraces reads in, one
     * Float64Array(n) in image row order out: per row the correctly rounded sum of |X|^2 over the request's frames divided by width, so
     * the same bits on every device and for every chunking - or, with `{db: true}`, the dB of that mean (not the mean of the dB values).
     * No image is rendered.  Only the sample detector has a mean.  Runs in the instance's request order; a malformed field rejects (and
     * reports `onerror`) and never resolves to an array.
     * @returns {Promise<{mean: Float64Array, width: number, n: number}>}
     */
    renderMean(m, opt) {
        return this._queued(() => this._meanRequest(m, opt), 'renderMean', r => ({ mean: r.mean, width: r.width, n: r.n }), ownStatus)
    }

    _meanRequest(m, opt) {
        return this._dbRequest(m, opt, 'a mean request needs a buffer', 'the mean power of the peak detector is not supported')
    }

    /** Synchronous form of renderMean (tests). */
    renderMeanSync(m, opt) { return addon().renderMeanSync(this._ctx, this._meanRequest(m, opt)) }

    /**
     * The exact band-power series of a request (sp_render_bandpower) - the zero-span / channel-power trace: the fields renderTraces
     * reads in plus `{bands}` - an array of [y0, y1] pairs or a flat Int32Array of them, half-open ranges of image rows with
     * 0 <= y0 <= y1 <= n, at most 64 (HipWorker.bandRows turns a frequency range into rows) - and one Float64Array(count * width) out,
     * band-major: bands[b * width + x] is the correctly rounded sum of |X|^2 of frame x over the rows of band b, the same bits on every
     * device and for every chunking - or, with `{db: true}`, the dB of that sum.  No image is rendered.  Only the sample detector has
     * band sums (status -4) and bad bands are refused (status -1), both before anything is rendered.  Runs in the instance's request
     * order; a malformed field rejects (and reports `onerror`) and never resolves to an array.
     * @returns {Promise<{bands: Float64Array, count: number, width: number, n: number}>}
     */
    renderBandPower(m, opt) {
        return this._queued(() => this._bandRequest(m, opt), 'renderBandPower',
            r => ({ bands: r.bands, count: r.count, width: r.width, n: r.n }), ownStatus)
    }

    _bandRequest(m, opt) {
        return this._dbRequest(m, opt, 'a band-power request needs a buffer', 'the band power of the peak detector is not supported',
            () => this._bandsField(m, opt, 'a band-power request'))
    }

    /** The `bands` field of a band-power or track request from `{bands}` of its options; what it refuses has status -1. */
    _bandsField(m, opt, who) {
        const given = opt && opt.bands
        if (!(Array.isArray(given) || ArrayBuffer.isView(given))) throw refusal(who + ' needs {bands}: [y0, y1] pairs', -1)
        const flat = Array.isArray(given) ? [].concat(...given) : Array.from(given)
        if (flat.length % 2 !== 0 || flat.length > 128) throw refusal('bands must be at most 64 [y0, y1] pairs', -1)
        for (let b = 0; b < flat.length; b += 2) {
            const y0 = flat[b], y1 = flat[b + 1]
            if (!Number.isInteger(y0) || !Number.isInteger(y1) || y0 < 0 || y1 < y0 || y1 > m.n) throw refusal('a band must satisfy 0 <= y0 <= y1 <= n', -1)
        }
        return { bands: Int32Array.from(flat) }
    }

    /** Synchronous form of renderBandPower (tests). */
    renderBandPowerSync(m, opt) { return addon().renderBandPowerSync(this._ctx, this._bandRequest(m, opt)) }

    /** sp_band_rows: the image rows [y0, y1) whose centre frequency (n/2 - y) / n lies in [fLo, fHi] cycles per sample (I/Q plans). */
    static bandRows(n, fLo, fHi) { return addon().bandRows(n, fLo, fHi) }

    /**
     * The peak track of a request (sp_render_track) - the peak search of a spectrum analyser per sweep, over time the
     * frequency-versus-time track of a transmitter: the fields renderTraces reads in plus `{bands}` as for renderBandPower, and two
     * arrays out, band-major: rows[b * width + x] is the strongest image row of frame x among the rows of band b that are not NaN (the
     * smallest among equal ones; -1 where there is none: an empty band, a capture shorter than n) and peaks[b * width + x] its |X|^2
     * bit for bit (NaN where there is none) - or, with `{db: true}`, the dB of it.  HipWorker.rowFreq turns a row into a frequency.
     * No image is rendered.  Only the sample detector has a track (status -4) and bad bands are refused (status -1), both before
     * anything is rendered.  Runs in the instance's request order; a malformed field rejects (and reports `onerror`) and never
     * resolves to arrays.
     * @returns {Promise<{rows: Int32Array, peaks: Float64Array, count: number, width: number, n: number}>}
     */
    renderTrack(m, opt) {
        return this._queued(() => this._trackRequest(m, opt), 'renderTrack',
            r => ({ rows: r.rows, peaks: r.peaks, count: r.count, width: r.width, n: r.n }), ownStatus)
    }

    _trackRequest(m, opt) {
        return this._dbRequest(m, opt, 'a track request needs a buffer', 'the peak track of the peak detector is not supported',
            () => this._bandsField(m, opt, 'a track request'))
    }

    /** Synchronous form of renderTrack (tests). */
    renderTrackSync(m, opt) { return addon().renderTrackSync(this._ctx, this._trackRequest(m, opt)) }

    /** The centre frequency of image row `row` of an n-point spectrum, (n/2 - row) / n cycles per sample; NaN for row -1 (I/Q plans). */
    static rowFreq(n, row) { return row < 0 ? NaN : (Math.floor(n / 2) - row) / n }

    /**
     * The occupancy counts of a request (sp_render_occupancy) - how often a frequency is in use and how much of a band is in use at a
     * time: the fields renderTraces reads in plus `{threshold, bands}` - `threshold` a power (|X|^2) for every image row or a
     * Float64Array(n) of one per row, `bands` as for renderBandPower (none: no frame counts) - and two Uint32Arrays out: rows[y] is the
     * number of frames whose |X|^2 at image row y is >= threshold[y] (rows[y] / width is the row's duty cycle) and, band-major,
     * frames[b * width + x] the number of rows of band b that reach theirs in frame x.  A NaN on either side is no hit, so a capture
     * shorter than n counts nothing.  The same words on every device and for every chunking.  No image is rendered.  Only the sample
     * detector has counts (status -4), and bad bands or a threshold that is neither a number nor n values are refused (status -1), all
     * before anything is rendered.  Runs in the instance's request order; a malformed field rejects (and reports `onerror`) and never
     * resolves to arrays.
     * @returns {Promise<{rows: Uint32Array, frames: Uint32Array, count: number, width: number, n: number}>}
     */
    renderOccupancy(m, opt) {
        return this._queued(() => this._occupancyRequest(m, opt), 'renderOccupancy',
            r => ({ rows: r.rows, frames: r.frames, count: r.count, width: r.width, n: r.n }), ownStatus)
    }

    _occupancyRequest(m, opt) {
        return this._plainRequest(m, 'an occupancy request needs a buffer', 'the occupancy counts of the peak detector are not supported', () => {
            const bands = opt && opt.bands !== undefined ? this._bandsField(m, opt, 'an occupancy request') : { bands: new Int32Array(0) }
            const given = opt && opt.threshold
            let threshold
            if (typeof given === 'number') threshold = new Float64Array(Number.isInteger(m.n) && m.n > 0 ? m.n : 0).fill(given)
            else if (given instanceof Float64Array) threshold = given
            else throw refusal('an occupancy request needs {threshold}: a power or a Float64Array of n powers', -1)
            if (threshold.length !== m.n) throw refusal('threshold must hold n values, one per image row', -1)
            return Object.assign({ threshold }, bands)
        })
    }

    /** Synchronous form of renderOccupancy (tests). */
    renderOccupancySync(m, opt) { return addon().renderOccupancySync(this._ctx, this._occupancyRequest(m, opt)) }

    /**
     * The picture of a worker message as ONE colour-index byte per pixel instead of RGBA (sp_render_index): index[j] is the entry of the
     * message's colour map pixel j of imageData.data shows, so the reply is a quarter of the size and js/consumers.js `recolour` redraws
     * it under another map without a render.  The message is a worker message (`detector: 'peak'` allowed; a colour map of more than 256
     * entries is refused with status -4); the `postMessage` path itself stays RGBA.  Runs in the instance's request order; a malformed
     * field rejects (and reports `onerror` with status -1) and never resolves to an image.
     * @returns {Promise<{index: Uint8Array, width: number, height: number, c_hist: number[], cB_hist: number[], dBfs_min: number,
     *          dBfs_max: number, gauge_mins: Uint8ClampedArray, gauge_maxs: Uint8ClampedArray, gauge_amps: Uint8ClampedArray}>}
     */
    renderIndexed(m) { return this._queued(() => this._indexRequest(m), 'renderIndex', r => this._wrapIndex(m, r), statusOrInvalid) }

    _indexRequest(m) {
        if (!(m && m.buffer)) throw refusal('an indexed request needs a buffer', -1)
        if (!Array.isArray(m.cmap)) throw refusal('an indexed request needs a colour map', -1)
        for (const k of ['n', 'width', 'block_norm', 'gain', 'range'])
            if (typeof m[k] !== 'number') throw refusal(`${k} must be a number, not ${JSON.stringify(m[k]) || String(m[k])}`, -1)
        return this._request(m)
    }

    _wrapIndex(m, r) {
        return {
            index: r.index, width: m.waterfall ? m.n : m.width, height: m.waterfall ? m.width : m.n,
            cB_hist: plainArray(r.cB_hist), c_hist: plainArray(r.c_hist), dBfs_min: r.dBfs_min, dBfs_max: r.dBfs_max,
            gauge_mins: new Uint8ClampedArray(r.gauge_mins), gauge_maxs: new Uint8ClampedArray(r.gauge_maxs),
            gauge_amps: new Uint8ClampedArray(r.gauge_amps),
        }
    }

    /**
     * The persistence spectrum of a worker message (sp_render_density): how many of the message's `width` frames showed colour index g in
     * image row y - density[y * lutLen + g], row y of the spectrogram and column n - 1 - y of the waterfall, the same array for both
     * layouts.  The message is renderIndexed's (`detector: 'peak'` allowed; a colour map of more than 256 entries is refused with status
     * -4).  Runs in the instance's request order; a malformed field rejects (and reports `onerror` with status -1) and never resolves to
     * counts.
     * @returns {Promise<{density: Uint32Array, n: number, lutLen: number, width: number}>}
     */
    renderDensity(m) { return this._queued(() => this._indexRequest(m), 'renderDensity', r => this._wrapDensity(r), statusOrInvalid) }

    _wrapDensity(r) { return { density: r.density, n: r.n, lutLen: r.lutLen, width: r.width } }

    /** Synchronous form of renderDensity (tests). */
    renderDensitySync(m) { return this._wrapDensity(addon().renderDensitySync(this._ctx, this._indexRequest(m))) }

    /** Synchronous form of renderIndexed (tests). */
    renderIndexedSync(m) { return this._wrapIndex(m, addon().renderIndexSync(this._ctx, this._indexRequest(m))) }

    /** Synchronous form of renderTraces (tests). */
    renderTracesSync(m) { return addon().renderTracesSync(this._ctx, this._tracesRequest(m)) }

    /** Synchronous form of renderNamed (tests). */
    renderNamedSync(o) { return this._wrap(o, addon().renderNamedSync(this._ctx, this._namedRequest(o))) }

    /** How many plans (table sets on the device) this worker's context has built so far. */
    planCreations() { return addon().planCreations(this._ctx) }

    /** Synchronous render of one message (used by tests and by callers that drive the GPUs themselves). */
    renderSync(m) { return this._wrap(m, addon().renderSync(this._ctx, this._request(m))) }

    /**
     * Worker.terminate(): queued requests are dropped, nothing is emitted any more, and the device context (stream, staging and
     * workspace buffers) is released as soon as the render that may be running on a libuv thread has returned.
     */
    terminate() {
        if (this._closed) return
        this._closed = true
        const ctx = this._ctx
        this._ctx = null
        if (ctx) addon().destroyContext(ctx)
    }
}

/** A constructor bound to one device, for `workerOrUrl: HipWorker.onDevice(3)`. */
HipWorker.onDevice = (device) => class extends HipWorker { constructor() { super({ device }) } }
HipWorker.deviceCount = () => addon().deviceCount()
/** The peak detector's sub-frame rule for a request's shape (sp_peak_subframes): {subframes: M, lastColumnCount}. */
HipWorker.peakSubframes = (format, n, nbytes, width) => addon().peakSubframes(addon().parseFormat(String(format)).id, n, nbytes, width)
/**
 * An ArrayBuffer in page-locked host memory.  A message whose `buffer` is one of these is copied to the GPU at the full rate of
 * the host link (pageable memory goes through the runtime's staging copies at less than half of it); js/render_file.js cuts its
 * slices into such buffers, where the reference's SampleView.slice copies into a plain one (lib/samples.js:253-258).
 */
HipWorker.allocBuffer = (nbytes) => addon().allocBuffer(nbytes)

module.exports = { HipWorker, packLut, plainArray, detectorId }
