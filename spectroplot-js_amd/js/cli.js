#!/usr/bin/env node
'use strict'
/**
 * Headless render of an I/Q capture to an image file through the GPUs — the data half of the reference's processData
 * (lib/spectroplot.js:1096-1285) without a browser:
 *
 *   node spectroplot-js_amd/js/cli.js capture_433.92M_250k.cu8 --n 1024 --width 2048 [--format cu8] [--window blackmanHarris]
 *        [--cmap cube1|viridis|plasma|inferno|magma|hot|afmhot|gist_heat|sox|naive|grayscale|roentgen|phosphor|parabola] [--gain 6] [--range 30] [--workers N] [--waterfall] [--lr] [--detector sample|peak]
 *        [--full] [--traces traces.json] [--index index.pgm] [--density density.pgm] [--power power.f64] [--power-db db.f64]
 *        [--mean mean.f64] [--mean-db mean_db.f64]
 *        [--bandpower bands.f64] [--bandpower-db bands_db.f64] [--bands Y0:Y1,...] [--band-freqs LO:HI,...]
 *        [--track-rows rows.i32] [--track-power peaks.f64] [--track-db peaks_db.f64]
 *        [--occupancy-rows rows.u32] [--occupancy-frames frames.u32] [--threshold P | --threshold-over-mean K]
 *        --out image.ppm
 *   node spectroplot-js_amd/js/cli.js a.cu8 b.cu8 c.cs16 ... --n 1024 --width 2048 [options] --out-dir DIR
 *
 * Batch mode (--out-dir): one image per capture, DIR/<capture's file name>.ppm (or .rgba with --rgba), the same bytes a single-file
 * run writes for it.  Captures are grouped by format (each file's extension, or --format) and every group is rendered with ONE native
 * call (renderMany -> sp_render_batch).  --full is for single-file runs.
 *
 * --traces FILE (single-file runs, sample detector): the per-bin min-hold / max-hold traces of the same request over the whole capture
 * (HipWorker.renderTraces -> sp_render_traces) as JSON beside the image: {n, width, trace_min: [n], trace_max: [n]} in image row order
 * (row y of the spectrogram, column n - 1 - y of the waterfall); a value JSON cannot hold travels as the string 'Infinity' / '-Infinity'.
 *
 * --index FILE (single-file runs): the same request over the whole capture as an indexed image (HipWorker.renderIndexed ->
 * sp_render_index), written beside the image as a binary PGM (P5, maxval 255): one colour-index byte per pixel, rows as the image's.
 *
 * --density FILE (single-file runs): the persistence spectrum of the same request over the whole capture (HipWorker.renderDensity ->
 * sp_render_density), written as a binary PGM (P5, maxval 65535, big-endian): lut_len columns x n rows, row y the image row's counts
 * per colour index, each value min(count, 65535).
 *
 * --power FILE / --power-db FILE (single-file runs, sample detector): the numeric spectrogram of the same request over the whole capture
 * (HipWorker.renderPower -> sp_render_power) as raw little-endian f64, width * n values, frame-major: |X|^2 (or, for --power-db, the dB
 * value 5 log10 |X|^2 + block_norm's dB) of frame x at value x * n + y, y the image row.
 *
 * --mean FILE / --mean-db FILE (single-file runs, sample detector): the exact mean-power trace of the same request over the whole capture
 * (HipWorker.renderMean -> sp_render_mean) as raw little-endian f64, n values in image row order: per row the correctly rounded sum of
 * |X|^2 over the frames divided by width (or, for --mean-db, the dB of that mean).
 *
 * --bandpower FILE / --bandpower-db FILE (single-file runs, sample detector): the exact band-power series of the same request over the
 * whole capture (HipWorker.renderBandPower -> sp_render_bandpower) as raw little-endian f64, count * width values, band-major: per band
 * and frame the correctly rounded sum of |X|^2 over the band's image rows (or, for --bandpower-db, the dB of that sum).  The bands are
 * --bands Y0:Y1,... (half-open ranges of image rows) followed by --band-freqs LO:HI,... (cycles per sample, -0.5 .. 0.5, turned into
 * rows by sp_band_rows: row y is centred on (n/2 - y) / n); at most 64 in all.
 *
 * --track-rows FILE / --track-power FILE / --track-db FILE (single-file runs, sample detector): the peak track of the same request over
 * the whole capture (HipWorker.renderTrack -> sp_render_track) for the bands of --bands / --band-freqs, count * width values each,
 * band-major: per band and frame the strongest image row that is not a NaN, the smallest among equal ones, as raw little-endian int32
 * (-1 where the band holds no value), its |X|^2 as raw little-endian f64 (NaN there), or for --track-db the dB of it.
 *
 * --occupancy-rows FILE / --occupancy-frames FILE (single-file runs, sample detector): the occupancy counts of the same request over the
 * whole capture (HipWorker.renderOccupancy -> sp_render_occupancy) as raw little-endian uint32: n values, per image row the frames whose
 * |X|^2 is >= the row's threshold, or count * width values, band-major, per band of --bands / --band-freqs and frame the rows that reach
 * theirs.  The threshold is --threshold P, one power for all rows, or --threshold-over-mean K: threshold[y] = K * mean[y], the exact
 * mean-power trace of the same request (one HipWorker.renderMean first, one multiply per row) - the noise-relative form.
 *
 * The format defaults to the file extension (lib/parseFreqRate.js:58-70), the worker count to the number of visible GPUs.
 * Output: binary PPM (P6, alpha dropped) or, with --out *.rgba, the raw RGBA bytes exactly as the reference's canvas holds them.
 * --full composes the plot the reference shows around the spectrogram (js/raster.js): amplitude and min/max gauge strips above it, to
 * its right the dB scale (colour ramp, tick marks) with the two histogram outlines over it (filled and stroked without anti-aliasing);
 * only the text labels need a canvas.
 */
const fs = require('fs')
const path = require('path')
const { renderSliced, renderMany, parseFormat, parseFreqRate, HipWorker, composePlot, cmapByName } = require('./index.js')

function writeImage(img, out) {
    if (out.endsWith('.rgba')) {
        fs.writeFileSync(out, Buffer.from(img.data.buffer, img.data.byteOffset, img.data.byteLength))
        return
    }
    const rgb = Buffer.alloc(img.width * img.height * 3)
    for (let p = 0, q = 0; p < img.data.length; p += 4) { rgb[q++] = img.data[p]; rgb[q++] = img.data[p + 1]; rgb[q++] = img.data[p + 2] }
    fs.writeFileSync(out, Buffer.concat([Buffer.from(`P6\n${img.width} ${img.height}\n255\n`), rgb]))
}

function readCapture(file) {
    const bytes = fs.readFileSync(file)
    return bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
}

// the bands of --bands and --band-freqs, in that order, as [y0, y1] pairs
function parseBands(opt, n, who = '--bandpower') {
    const pairs = (text, num) => String(text).split(',').filter(s => s.length).map(s => {
        const p = s.split(':')
        if (p.length !== 2 || !p.every(v => v.trim().length && Number.isFinite(num(v)))) throw new Error(`bad band '${s}': A:B expected`)
        return p.map(num)
    })
    const bands = opt.bands === undefined ? [] : pairs(opt.bands, Number)
    if (opt['band-freqs'] !== undefined) for (const [lo, hi] of pairs(opt['band-freqs'], Number)) bands.push(HipWorker.bandRows(n, lo, hi))
    if (!bands.length) throw new Error(who + ' needs --bands Y0:Y1,... and / or --band-freqs LO:HI,...')
    return bands
}

// {threshold} of an occupancy request: --threshold P, or K times the request's own mean trace (a promise then)
function occupancyThreshold(opt, worker, message, who) {
    const number = (name) => {
        const v = Number(opt[name])
        if (!String(opt[name]).trim().length || Number.isNaN(v)) throw new Error(`--${name} needs a number`)
        return v
    }
    if ((opt.threshold === undefined) === (opt['threshold-over-mean'] === undefined)) throw new Error(who + ' needs either --threshold P or --threshold-over-mean K')
    if (opt.threshold !== undefined) return { threshold: number('threshold') }
    const k = number('threshold-over-mean')
    return worker.renderMean(message).then(r => ({ threshold: r.mean.map(v => k * v) }))
}

// a typed array's bytes as they are (every host this runs on is little-endian)
const raw = a => Buffer.from(a.buffer, a.byteOffset, a.byteLength)

// --NAME FILE / --NAME-db FILE: raw f64 of the reply's `field`; `own(opt, n)`: the kind's options beside `db`
const f64Outputs = (name, method, field, own) => [false, true].map(db => ({ option: db ? name + '-db' : name, method,
    options: (opt, n) => Object.assign({ db }, own && own(opt, n)), bytes: r => raw(r[field]) }))

// The side outputs of a single-file run, in the order they are written.  `picture`: the request carries the end-forced colour map and
// `waterfall`, as the image's does; `method` of HipWorker gets the message and `options(opt, n, worker, message)` - or what that promises,
// where the options take a request of their own -; `bytes(reply, n, width)` is the file.
const SIDE_OUTPUTS = [
    { option: 'traces', method: 'renderTraces', bytes: (t, n, width) => {
        const plain = a => Array.from(a, v => Number.isFinite(v) ? v : String(v))
        return JSON.stringify({ n, width, trace_min: plain(t.trace_min), trace_max: plain(t.trace_max) })
    } },
    { option: 'index', picture: true, method: 'renderIndexed',
        bytes: r => Buffer.concat([Buffer.from(`P5\n${r.width} ${r.height}\n255\n`), raw(r.index)]) },
    { option: 'density', picture: true, method: 'renderDensity', bytes: r => {                 // raw counts, saturated at 65535
        const body = Buffer.alloc(2 * r.density.length)
        for (let i = 0; i < r.density.length; i++) body.writeUInt16BE(r.density[i] < 65535 ? r.density[i] : 65535, 2 * i)
        return Buffer.concat([Buffer.from(`P5\n${r.lutLen} ${r.n}\n65535\n`), body])
    } },
    ...f64Outputs('power', 'renderPower', 'power'),                    // width * n values, frame-major
    ...f64Outputs('mean', 'renderMean', 'mean'),                       // n values
    ...f64Outputs('bandpower', 'renderBandPower', 'bands', (opt, n) => ({ bands: parseBands(opt, n) })),   // count * width values, band-major
    // the peak track, count * width values each, band-major: the rows as int32, their power and its dB as f64
    { option: 'track-rows', method: 'renderTrack', options: (opt, n) => ({ bands: parseBands(opt, n, '--track-rows') }), bytes: r => raw(r.rows) },
    { option: 'track-power', method: 'renderTrack', options: (opt, n) => ({ bands: parseBands(opt, n, '--track-power') }), bytes: r => raw(r.peaks) },
    { option: 'track-db', method: 'renderTrack', options: (opt, n) => ({ db: true, bands: parseBands(opt, n, '--track-db') }), bytes: r => raw(r.peaks) },
    // the occupancy counts as uint32: n values per row, and count * width values, band-major
    { option: 'occupancy-rows', method: 'renderOccupancy', options: (opt, n, worker, message) =>
        occupancyThreshold(opt, worker, message, '--occupancy-rows'), bytes: r => raw(r.rows) },
    { option: 'occupancy-frames', method: 'renderOccupancy', options: (opt, n, worker, message) => {
        const bands = parseBands(opt, n, '--occupancy-frames')
        return Promise.resolve(occupancyThreshold(opt, worker, message, '--occupancy-frames')).then(t => Object.assign({ bands }, t))
    }, bytes: r => raw(r.frames) },
]

// one side output: one request over the whole capture on one worker, with the taper and block_norm the image's request resolves to
function writeSide(kind, buffer, format, n, width, opt) {
    const native = require(path.join(__dirname, '..', 'lib', 'spectroplot_hip.node'))
    const w = native.window(native.namedResolve(String(opt.window), String(opt.cmap)).window, n)
    const message = { buffer, format, n, width, windowc: w.window, block_norm: 1.0 / w.weight, gain: parseFloat(opt.gain),
        range: parseFloat(opt.range), channelMode: !!opt.channelMode, detector: opt.detector }
    if (kind.picture) {
        const cmap = cmapByName(String(opt.cmap)).map(c => c.slice())
        cmap[0] = [0, 0, 0]; cmap[cmap.length - 1] = [255, 255, 255]                    // lib/spectroplot.js:1129-1130
        Object.assign(message, { cmap, waterfall: !!opt.waterfall })
    }
    const worker = new HipWorker()
    return new Promise(resolve => resolve(kind.options && kind.options(opt, n, worker, message)))
        .then(options => worker[kind.method](message, options)).then(r => {
            worker.terminate()
            fs.writeFileSync(opt[kind.option], kind.bytes(r, n, width))
        }, e => { worker.terminate(); throw e })
}

// --out-dir: the captures grouped by format, each group in one batch; the option names resolve as the single-file run's do
function mainBatch(files, opt) {
    const native = require(path.join(__dirname, '..', 'lib', 'spectroplot_hip.node'))
    const n = parseInt(opt.n, 10), width = parseInt(opt.width, 10)
    const resolved = native.namedResolve(String(opt.window), String(opt.cmap))   // lookup rules of lib/utils.js:25-40, with the defaults
    const cmap = cmapByName(String(opt.cmap))
    fs.mkdirSync(opt['out-dir'], { recursive: true })
    const groups = new Map()
    for (const file of files) {
        const format = opt.format || parseFormat(file)
        if (!groups.has(format)) groups.set(format, [])
        groups.get(format).push(file)
    }
    let chain = Promise.resolve()
    for (const [format, group] of groups) {
        chain = chain.then(() => renderMany({ buffers: group.map(readCapture), format, n, width, window: resolved.window, cmap,
            gain: parseFloat(opt.gain), range: parseFloat(opt.range), channelMode: !!opt.channelMode, waterfall: !!opt.waterfall,
            detector: opt.detector }))                                  // (batches refuse 'peak')
            .then(imgs => imgs.forEach((img, k) => {
                const out = path.join(opt['out-dir'], path.basename(group[k]) + (opt.rgba ? '.rgba' : '.ppm'))
                writeImage(img, out)
                console.log(`${group[k]}: ${format} -> ${out} (${img.width} x ${img.height}), dBfs ${img.dBfs_min.toFixed(2)} .. ${img.dBfs_max.toFixed(2)}`)
            }))
    }
    return chain
}

function main(argv) {
    const opt = { n: 512, width: 1024, window: 'blackmanHarris', cmap: 'cube1', gain: 6, range: 30, out: 'spectrogram.ppm' }
    let file = null
    const files = []
    for (let i = 0; i < argv.length; i++) {
        const a = argv[i]
        if (a === '--waterfall') opt.waterfall = true
        else if (a === '--full') opt.full = true
        else if (a === '--lr') opt.channelMode = true
        else if (a === '--rgba') opt.rgba = true
        else if (a.startsWith('--')) opt[a.slice(2)] = argv[++i]
        else { file = a; files.push(a) }
    }
    if (opt['out-dir'] !== undefined) {
        if (!files.length) { console.error('usage: cli.js <capture> ... --n N --width W [options] --out-dir DIR'); process.exit(2) }
        return mainBatch(files, opt)
    }
    if (!file) { console.error('usage: cli.js <capture> --n N --width W [options] --out image.ppm'); process.exit(2) }
    const bytes = fs.readFileSync(file)
    const buffer = bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
    const format = opt.format || parseFormat(file)
    const n = parseInt(opt.n, 10), width = parseInt(opt.width, 10)
    const fr = parseFreqRate(file)
    const t0 = Date.now()
    return renderSliced({ buffer, format, n, width, workers: opt.workers ? parseInt(opt.workers, 10) : HipWorker.deviceCount(),
        // the option names travel as they are: the library resolves them as the reference's caller does (sp_render_named)
        byName: true, window: String(opt.window), cmap: String(opt.cmap), gain: parseFloat(opt.gain), range: parseFloat(opt.range), channelMode: !!opt.channelMode, waterfall: !!opt.waterfall,
        detector: opt.detector })                                       // 'peak': max hold between columns; anything unknown is an error
        .then(img => {
            if (opt.full) {
                const cmap = cmapByName(String(opt.cmap)).map(c => c.slice())
                cmap[0] = [0, 0, 0]; cmap[cmap.length - 1] = [255, 255, 255]                    // lib/spectroplot.js:1129-1130
                const plot = composePlot(img, { cmap, gain: parseFloat(opt.gain), range: parseFloat(opt.range), n, waterfall: !!opt.waterfall })
                if (opt.out.endsWith('.rgba')) fs.writeFileSync(opt.out, Buffer.from(plot.surface.data.buffer))
                else fs.writeFileSync(opt.out, plot.surface.toPPM())
                img = { width: plot.surface.width, height: plot.surface.height, dBfs_min: img.dBfs_min, dBfs_max: img.dBfs_max }
            } else {
                writeImage(img, opt.out)
            }
            console.log(`${file}: ${format}, centre ${fr.freq} Hz, rate ${fr.rate} Hz -> ${opt.out} (${img.width} x ${img.height}), ` +
                `dBfs ${img.dBfs_min.toFixed(2)} .. ${img.dBfs_max.toFixed(2)}, ${Date.now() - t0} ms`)
        })
        .then(() => SIDE_OUTPUTS.reduce((done, kind) => done.then(() => opt[kind.option] === undefined ? null
            : writeSide(kind, buffer, format, n, width, opt)), Promise.resolve()))
}

// (an explicit exit: Node 12 can crash while it tears its environment down when finalizers of collected reply buffers are
// still queued - after all output, but with status 139; process.exit() does not take that path)
main(process.argv.slice(2)).then(() => process.exit(0), e => { console.error(e.message || e); process.exit(1) })
