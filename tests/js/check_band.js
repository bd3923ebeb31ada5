'use strict'
/**
 * GPU: the exact band-power series through the Node layer.  argv[2] is a directory pytest has filled (tests/test_node_band_gpu.py):
 * cases.json and, per case, the capture and the expected arrays (raw f64, band-major, from tests/bandref.py).  Every case goes through
 * HipWorker.renderBandPower (asynchronous and synchronous, with and without `db`), the addon's renderBandPower / renderBandPowerSync /
 * bandRows and `cli.js --bandpower` / `--bandpower-db` with --bands and --band-freqs; NaN positions must agree and every other value is
 * compared bit for bit.  A peak detector is refused with status -4 and bad bands with -1, before anything is rendered.
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
function f64(file) {
    const b = fs.readFileSync(file)
    return new Float64Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength))
}
function check(what, got, want, c, count) {
    if (!got || got.width !== c.width || got.n !== c.n || got.count !== count || want.length !== count * c.width || !same(got.bands, want))
        throw new Error(`${what}: the band series differ`)
}

async function main(dir) {
    const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'))
    const worker = new HipWorker({ device: 0 })
    const ctx = native.createContext(0)
    for (const c of cases) {
        const file = path.join(dir, c.file)
        const bytes = fs.readFileSync(file)
        const buffer = bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
        const want = { bands: f64(path.join(dir, c.id + '.bands')), db: f64(path.join(dir, c.id + '.db')) }
        // sp_band_rows through the addon and the worker
        c.freqs.forEach(([lo, hi], k) => {
            const a = native.bandRows(c.n, lo, hi), b = HipWorker.bandRows(c.n, lo, hi)
            if (a[0] !== c.rowsOfFreqs[k][0] || a[1] !== c.rowsOfFreqs[k][1] || b[0] !== a[0] || b[1] !== a[1])
                throw new Error(`${c.id}: bandRows(${c.n}, ${lo}, ${hi}) = ${a}, want ${c.rowsOfFreqs[k]}`)
        })
        for (const bad of [[6, 0, 0], [c.n, 0.2, 0.1], [c.n, NaN, 0]]) {
            let thrown = null
            try { native.bandRows(...bad) } catch (e) { thrown = e }
            if (!thrown) throw new Error(`bandRows(${bad}) did not throw`)
        }
        const bands = c.rows.concat(c.rowsOfFreqs), count = bands.length
        const w = native.window(c.window, c.n)
        const message = { buffer, format: c.format, n: c.n, windowc: Array.from(w.window), block_norm: 1.0 / w.weight, gain: c.gain,
            range: c.range, width: c.width, channelMode: c.channelMode, cmap: [[0, 0, 0], [255, 255, 255]], offset: 0 }
        check(`${c.id} renderBandPower`, await worker.renderBandPower(message, { bands }), want.bands, c, count)
        check(`${c.id} renderBandPower {db: false}`, await worker.renderBandPower(message, { bands, db: false }), want.bands, c, count)
        check(`${c.id} renderBandPower {db: true}`, await worker.renderBandPower(message, { bands, db: true }), want.db, c, count)
        check(`${c.id} renderBandPower (flat Int32Array)`, await worker.renderBandPower(message, { bands: Int32Array.from([].concat(...bands)) }),
            want.bands, c, count)
        check(`${c.id} renderBandPowerSync (worker)`, worker.renderBandPowerSync(message, { bands }), want.bands, c, count)
        check(`${c.id} renderBandPowerSync (worker) {db: true}`, worker.renderBandPowerSync(message, { bands, db: true }), want.db, c, count)
        const req = { format: native.parseFormat(c.format).id, buffer, n: c.n, width: c.width, windowc: w.window, block_norm: 1.0 / w.weight,
            gain: c.gain, range: c.range, channelMode: c.channelMode, db: false, bands: Int32Array.from([].concat(...bands)) }
        check(`${c.id} renderBandPowerSync (addon)`, native.renderBandPowerSync(ctx, req), want.bands, c, count)
        check(`${c.id} renderBandPowerSync (addon) db`, native.renderBandPowerSync(ctx, Object.assign({}, req, { db: true })), want.db, c, count)
        const viaCallback = await new Promise((resolve, reject) => native.renderBandPower(ctx, req, (err, r) => err ? reject(err) : resolve(r)))
        check(`${c.id} renderBandPower (addon)`, viaCallback, want.bands, c, count)
        const none = native.renderBandPowerSync(ctx, Object.assign({}, req, { bands: new Int32Array(0) }))
        if (none.count !== 0 || none.bands.length !== 0) throw new Error(`${c.id}: no bands did not give an empty reply`)
        // the addon hands the library's refusal on: status -1 for bands it does not take
        for (const rows of [[0, c.n + 1], [4, 3], [-1, 2], new Array(130).fill(0)]) {
            let thrown = null
            try { native.renderBandPowerSync(ctx, Object.assign({}, req, { bands: Int32Array.from(rows) })) } catch (e) { thrown = e }
            if (!thrown || thrown.status !== -1) throw new Error(`${c.id} addon: bands ${rows.slice(0, 4)} were not refused with -1`)
        }
        for (const rows of [Int32Array.from([0, 1, 2]), undefined, [0, 1], Float64Array.from([0, 1])]) {   // no Int32Array of pairs
            let threw = false
            try { native.renderBandPowerSync(ctx, Object.assign({}, req, { bands: rows })) } catch (e) { threw = true }
            if (!threw) throw new Error(`${c.id} addon: malformed bands did not throw`)
        }

        // cli.js --bandpower / --bandpower-db: raw little-endian f64, band-major; --bands first, then --band-freqs
        const outB = path.join(dir, c.id + '.bands.out'), outD = path.join(dir, c.id + '.db.out'), img = path.join(dir, c.id + '.rgba')
        execFileSync(process.execPath, [path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js'), file, '--format', c.format, '--n',
            String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain), '--range', String(c.range), '--workers', '1',
            ...(c.channelMode ? ['--lr'] : []), '--bands', c.rows.map(r => r.join(':')).join(','), '--band-freqs',
            c.freqs.map(r => r.join(':')).join(','), '--bandpower', outB, '--bandpower-db', outD, '--out', img], { stdio: 'pipe' })
        if (fs.statSync(outB).size !== 8 * count * c.width || fs.statSync(outD).size !== 8 * count * c.width) throw new Error(`${c.id} cli: file size`)
        if (!same(f64(outB), want.bands)) throw new Error(`${c.id} cli --bandpower: the series differ`)
        if (!same(f64(outD), want.db)) throw new Error(`${c.id} cli --bandpower-db: the series differ`)
        if (fs.statSync(img).size !== 4 * c.n * c.width) throw new Error(`${c.id} cli: image size`)
        // ... --band-freqs alone
        execFileSync(process.execPath, [path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js'), file, '--format', c.format, '--n',
            String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain), '--range', String(c.range), '--workers', '1',
            ...(c.channelMode ? ['--lr'] : []), '--band-freqs', c.freqs.map(r => r.join(':')).join(','), '--bandpower', outB, '--out', img],
        { stdio: 'pipe' })
        if (!same(f64(outB), want.bands.subarray(c.rows.length * c.width))) throw new Error(`${c.id} cli --band-freqs alone: the series differ`)

        // the two refusals: a peak detector -4, bad bands -1, in onerror / a throw and never in an array
        const refusals = [[{ detector: 'peak' }, { bands }, -4], [{}, { bands: [[0, c.n + 1]] }, -1], [{}, { bands: [[5, 4]] }, -1],
            [{}, { bands: [[0, 1.5]] }, -1], [{}, { bands: new Array(65).fill([0, 1]) }, -1], [{}, {}, -1], [{}, { bands: [0, 1, 2] }, -1]]
        for (const [extra, opt, status] of refusals) {
            let events = 0, seen
            worker.onerror = (e) => { events++; seen = e.status }
            let got = null, err = null
            try { got = await worker.renderBandPower(Object.assign({}, message, extra), opt) } catch (e) { err = e }
            await new Promise(r => setImmediate(r))
            worker.onerror = null
            if (got !== null || !err || err.status !== status || events !== 1 || seen !== status)
                throw new Error(`${c.id}: ${JSON.stringify([extra, opt])} was not refused with ${status} (${got}, ${err && err.status}, ${events}, ${seen})`)
            let thrown = null
            try { worker.renderBandPowerSync(Object.assign({}, message, extra), opt) } catch (e) { thrown = e }
            if (!thrown || thrown.status !== status) throw new Error(`${c.id}: ${JSON.stringify([extra, opt])} (sync) was not refused with ${status}`)
        }
        let threw = false
        try { native.renderBandPowerSync(ctx, { format: 'cu8', buffer, n: c.n, width: c.width }) } catch (e) { threw = true }
        if (!threw) throw new Error('addon: a request without its numbers did not throw')
        check(`${c.id} after the refusals`, await worker.renderBandPower(message, { bands }), want.bands, c, count)
    }
    worker.terminate()
    native.destroyContext(ctx)
    console.log(`band ok: ${cases.length} cases`)
}

main(process.argv[2]).then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
