'use strict'
/**
 * GPU: the peak track through the Node layer.  argv[2] is a directory pytest has filled (tests/test_node_track_gpu.py): cases.json and,
 * per case, the capture and the expected arrays (raw int32 rows, raw f64 peaks and their dB, band-major, from tests/trackref.py).  Every
 * case goes through HipWorker.renderTrack (asynchronous and synchronous, with and without `db`), the addon's renderTrack /
 * renderTrackSync and `cli.js --track-rows` / `--track-power` / `--track-db` with --bands and --band-freqs; the rows must be equal, NaN
 * positions must agree and every other value is compared bit for bit.  A peak detector is refused with status -4 and bad bands with
 * -1, before anything is rendered.
 */
const fs = require('fs')
const path = require('path')
const { execFileSync } = require('child_process')
const { HipWorker } = require('../../spectroplot-js_amd/js')
const native = require('../../spectroplot-js_amd/lib/spectroplot_hip.node')

function bits(a) { return new BigUint64Array(a.buffer, a.byteOffset, a.length) }
function same(a, b) {
    if (!(a instanceof Float64Array) || a.length !== b.length) return false
    const x = bits(a), y = bits(b)
    for (let i = 0; i < x.length; i++) {
        if (Number.isNaN(a[i]) !== Number.isNaN(b[i])) return false
        if (!Number.isNaN(a[i]) && x[i] !== y[i]) return false
    }
    return true
}
function sameRows(a, b) {
    if (!(a instanceof Int32Array) || a.length !== b.length) return false
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false
    return true
}
function read(file, Type) {
    const b = fs.readFileSync(file)
    return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength))
}
function check(what, got, rows, peaks, c, count) {
    if (!got || got.width !== c.width || got.n !== c.n || got.count !== count || rows.length !== count * c.width || !sameRows(got.rows, rows))
        throw new Error(`${what}: the rows differ`)
    if (!same(got.peaks, peaks)) throw new Error(`${what}: the peaks differ`)
}

async function main(dir) {
    const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'))
    const worker = new HipWorker({ device: 0 })
    const ctx = native.createContext(0)
    for (const c of cases) {
        const file = path.join(dir, c.file)
        const bytes = fs.readFileSync(file)
        const buffer = bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
        const want = { rows: read(path.join(dir, c.id + '.rows'), Int32Array), peaks: read(path.join(dir, c.id + '.peaks'), Float64Array),
            db: read(path.join(dir, c.id + '.db'), Float64Array) }
        // a row's frequency: the inverse of bandRows for one row, NaN for "no row"
        for (const y of [0, 1, c.n / 2, c.n - 1]) {
            const f = HipWorker.rowFreq(c.n, y), r = HipWorker.bandRows(c.n, f, f)
            if (f !== (c.n / 2 - y) / c.n || r[0] !== y || r[1] !== y + 1) throw new Error(`${c.id}: rowFreq(${c.n}, ${y}) = ${f}`)
        }
        if (!Number.isNaN(HipWorker.rowFreq(c.n, -1))) throw new Error('rowFreq(n, -1) is not NaN')
        const bands = c.rows.concat(c.rowsOfFreqs), count = bands.length
        const w = native.window(c.window, c.n)
        const message = { buffer, format: c.format, n: c.n, windowc: Array.from(w.window), block_norm: 1.0 / w.weight, gain: c.gain,
            range: c.range, width: c.width, channelMode: c.channelMode, cmap: [[0, 0, 0], [255, 255, 255]], offset: 0 }
        check(`${c.id} renderTrack`, await worker.renderTrack(message, { bands }), want.rows, want.peaks, c, count)
        check(`${c.id} renderTrack {db: false}`, await worker.renderTrack(message, { bands, db: false }), want.rows, want.peaks, c, count)
        check(`${c.id} renderTrack {db: true}`, await worker.renderTrack(message, { bands, db: true }), want.rows, want.db, c, count)
        check(`${c.id} renderTrack (flat Int32Array)`, await worker.renderTrack(message, { bands: Int32Array.from([].concat(...bands)) }),
            want.rows, want.peaks, c, count)
        check(`${c.id} renderTrackSync (worker)`, worker.renderTrackSync(message, { bands }), want.rows, want.peaks, c, count)
        check(`${c.id} renderTrackSync (worker) {db: true}`, worker.renderTrackSync(message, { bands, db: true }), want.rows, want.db, c, count)
        const req = { format: native.parseFormat(c.format).id, buffer, n: c.n, width: c.width, windowc: w.window, block_norm: 1.0 / w.weight,
            gain: c.gain, range: c.range, channelMode: c.channelMode, db: false, bands: Int32Array.from([].concat(...bands)) }
        check(`${c.id} renderTrackSync (addon)`, native.renderTrackSync(ctx, req), want.rows, want.peaks, c, count)
        check(`${c.id} renderTrackSync (addon) db`, native.renderTrackSync(ctx, Object.assign({}, req, { db: true })), want.rows, want.db, c, count)
        const viaCallback = await new Promise((resolve, reject) => native.renderTrack(ctx, req, (err, r) => err ? reject(err) : resolve(r)))
        check(`${c.id} renderTrack (addon)`, viaCallback, want.rows, want.peaks, c, count)
        const none = native.renderTrackSync(ctx, Object.assign({}, req, { bands: new Int32Array(0) }))
        if (none.count !== 0 || none.rows.length !== 0 || none.peaks.length !== 0) throw new Error(`${c.id}: no bands did not give an empty reply`)
        // the addon hands the library's refusal on: status -1 for bands it does not take
        for (const rows of [[0, c.n + 1], [4, 3], [-1, 2], new Array(130).fill(0)]) {
            let thrown = null
            try { native.renderTrackSync(ctx, Object.assign({}, req, { bands: Int32Array.from(rows) })) } catch (e) { thrown = e }
            if (!thrown || thrown.status !== -1) throw new Error(`${c.id} addon: bands ${rows.slice(0, 4)} were not refused with -1`)
        }
        for (const rows of [Int32Array.from([0, 1, 2]), undefined, [0, 1], Float64Array.from([0, 1])]) {   // no Int32Array of pairs
            let threw = false
            try { native.renderTrackSync(ctx, Object.assign({}, req, { bands: rows })) } catch (e) { threw = true }
            if (!threw) throw new Error(`${c.id} addon: malformed bands did not throw`)
        }

        // cli.js --track-rows / --track-power / --track-db: raw little-endian int32 and f64, band-major; --bands first, then --band-freqs
        const outR = path.join(dir, c.id + '.rows.out'), outP = path.join(dir, c.id + '.peaks.out'), outD = path.join(dir, c.id + '.db.out')
        const img = path.join(dir, c.id + '.rgba')
        execFileSync(process.execPath, [path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js'), file, '--format', c.format, '--n',
            String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain), '--range', String(c.range), '--workers', '1',
            ...(c.channelMode ? ['--lr'] : []), '--bands', c.rows.map(r => r.join(':')).join(','), '--band-freqs',
            c.freqs.map(r => r.join(':')).join(','), '--track-rows', outR, '--track-power', outP, '--track-db', outD, '--out', img], { stdio: 'pipe' })
        if (fs.statSync(outR).size !== 4 * count * c.width || fs.statSync(outP).size !== 8 * count * c.width
            || fs.statSync(outD).size !== 8 * count * c.width) throw new Error(`${c.id} cli: file size`)
        if (!sameRows(read(outR, Int32Array), want.rows)) throw new Error(`${c.id} cli --track-rows: the rows differ`)
        if (!same(read(outP, Float64Array), want.peaks)) throw new Error(`${c.id} cli --track-power: the peaks differ`)
        if (!same(read(outD, Float64Array), want.db)) throw new Error(`${c.id} cli --track-db: the peaks differ`)
        if (fs.statSync(img).size !== 4 * c.n * c.width) throw new Error(`${c.id} cli: image size`)
        // ... --band-freqs alone
        execFileSync(process.execPath, [path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js'), file, '--format', c.format, '--n',
            String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain), '--range', String(c.range), '--workers', '1',
            ...(c.channelMode ? ['--lr'] : []), '--band-freqs', c.freqs.map(r => r.join(':')).join(','), '--track-rows', outR, '--out', img],
        { stdio: 'pipe' })
        if (!sameRows(read(outR, Int32Array), want.rows.subarray(c.rows.length * c.width))) throw new Error(`${c.id} cli --band-freqs alone: the rows differ`)

        // the two refusals: a peak detector -4, bad bands -1, in onerror / a throw and never in an array
        const refusals = [[{ detector: 'peak' }, { bands }, -4], [{}, { bands: [[0, c.n + 1]] }, -1], [{}, { bands: [[5, 4]] }, -1],
            [{}, { bands: [[0, 1.5]] }, -1], [{}, { bands: new Array(65).fill([0, 1]) }, -1], [{}, {}, -1], [{}, { bands: [0, 1, 2] }, -1]]
        for (const [extra, opt, status] of refusals) {
            let events = 0, seen
            worker.onerror = (e) => { events++; seen = e.status }
            let got = null, err = null
            try { got = await worker.renderTrack(Object.assign({}, message, extra), opt) } catch (e) { err = e }
            await new Promise(r => setImmediate(r))
            worker.onerror = null
            if (got !== null || !err || err.status !== status || events !== 1 || seen !== status)
                throw new Error(`${c.id}: ${JSON.stringify([extra, opt])} was not refused with ${status} (${got}, ${err && err.status}, ${events}, ${seen})`)
            let thrown = null
            try { worker.renderTrackSync(Object.assign({}, message, extra), opt) } catch (e) { thrown = e }
            if (!thrown || thrown.status !== status) throw new Error(`${c.id}: ${JSON.stringify([extra, opt])} (sync) was not refused with ${status}`)
        }
        let threw = false
        try { native.renderTrackSync(ctx, { format: 'cu8', buffer, n: c.n, width: c.width }) } catch (e) { threw = true }
        if (!threw) throw new Error('addon: a request without its numbers did not throw')
        check(`${c.id} after the refusals`, await worker.renderTrack(message, { bands }), want.rows, want.peaks, c, count)
    }
    worker.terminate()
    native.destroyContext(ctx)
    console.log(`track ok: ${cases.length} cases`)
}

main(process.argv[2]).then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
