'use strict'
/**
 * GPU: the exact mean-power trace through the Node layer.  argv[2] is a directory pytest has filled (tests/test_node_mean_gpu.py):
 * cases.json and, per case, the capture and the expected arrays (raw f64, from tests/meanref.py).  Every case goes through
 * HipWorker.renderMean (asynchronous and synchronous, with and without `db`), the addon's renderMeanSync and `cli.js --mean` /
 * `--mean-db`; NaN positions must agree and every other value is compared bit for bit.  A peak detector is refused with status -4 and
 * an unknown one with -1, before anything is rendered.
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
function check(what, got, want, c) {
    if (!got || got.width !== c.width || got.n !== c.n || want.length !== c.n || !same(got.mean, want)) throw new Error(`${what}: the mean differs`)
}

async function main(dir) {
    const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'))
    const worker = new HipWorker({ device: 0 })
    const ctx = native.createContext(0)
    for (const c of cases) {
        const file = path.join(dir, c.file)
        const bytes = fs.readFileSync(file)
        const buffer = bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
        const want = { mean: f64(path.join(dir, c.id + '.mean')), db: f64(path.join(dir, c.id + '.db')) }
        const w = native.window(c.window, c.n)
        const message = { buffer, format: c.format, n: c.n, windowc: Array.from(w.window), block_norm: 1.0 / w.weight, gain: c.gain,
            range: c.range, width: c.width, channelMode: c.channelMode, cmap: [[0, 0, 0], [255, 255, 255]], offset: 0 }
        check(`${c.id} renderMean`, await worker.renderMean(message), want.mean, c)
        check(`${c.id} renderMean {db: false}`, await worker.renderMean(message, { db: false }), want.mean, c)
        check(`${c.id} renderMean {db: true}`, await worker.renderMean(message, { db: true }), want.db, c)
        check(`${c.id} renderMeanSync (worker)`, worker.renderMeanSync(message), want.mean, c)
        check(`${c.id} renderMeanSync (worker) {db: true}`, worker.renderMeanSync(message, { db: true }), want.db, c)
        const req = { format: native.parseFormat(c.format).id, buffer, n: c.n, width: c.width, windowc: w.window, block_norm: 1.0 / w.weight,
            gain: c.gain, range: c.range, channelMode: c.channelMode, db: false }
        check(`${c.id} renderMeanSync (addon)`, native.renderMeanSync(ctx, req), want.mean, c)
        check(`${c.id} renderMeanSync (addon) db`, native.renderMeanSync(ctx, Object.assign({}, req, { db: true })), want.db, c)
        const viaCallback = await new Promise((resolve, reject) => native.renderMean(ctx, req, (err, r) => err ? reject(err) : resolve(r)))
        check(`${c.id} renderMean (addon)`, viaCallback, want.mean, c)
        // cli.js --mean / --mean-db: raw little-endian f64 beside the image
        const outM = path.join(dir, c.id + '.mean.out'), outD = path.join(dir, c.id + '.db.out'), img = path.join(dir, c.id + '.rgba')
        execFileSync(process.execPath, [path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js'), file, '--format', c.format, '--n',
            String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain), '--range', String(c.range), '--workers', '1',
            ...(c.channelMode ? ['--lr'] : []), '--mean', outM, '--mean-db', outD, '--out', img], { stdio: 'pipe' })
        if (fs.statSync(outM).size !== 8 * c.n || fs.statSync(outD).size !== 8 * c.n) throw new Error(`${c.id} cli: file size`)
        if (!same(f64(outM), want.mean)) throw new Error(`${c.id} cli --mean: the mean differs`)
        if (!same(f64(outD), want.db)) throw new Error(`${c.id} cli --mean-db: the mean differs`)
        if (fs.statSync(img).size !== 4 * c.n * c.width) throw new Error(`${c.id} cli: image size`)

        // the two refusals: a peak detector -4, an unknown one -1, in onerror / a throw and never in an array
        for (const [detector, status] of [['peak', -4], ['rms', -1]]) {
            let events = 0, seen
            worker.onerror = (e) => { events++; seen = e.status }
            let got = null, err = null
            try { got = await worker.renderMean(Object.assign({}, message, { detector })) } catch (e) { err = e }
            await new Promise(r => setImmediate(r))
            worker.onerror = null
            if (got !== null || !err || err.status !== status || events !== 1 || seen !== status)
                throw new Error(`${c.id}: detector ${detector} was not refused with ${status} (${got}, ${err && err.status}, ${events}, ${seen})`)
            let thrown = null
            try { worker.renderMeanSync(Object.assign({}, message, { detector })) } catch (e) { thrown = e }
            if (!thrown || thrown.status !== status) throw new Error(`${c.id}: detector ${detector} (sync) was not refused with ${status}`)
        }
        let threw = false
        try { native.renderMeanSync(ctx, { format: 'cu8', buffer, n: c.n, width: c.width }) } catch (e) { threw = true }
        if (!threw) throw new Error('addon: a request without its numbers did not throw')
        check(`${c.id} after the refusals`, await worker.renderMean(message), want.mean, c)
    }
    worker.terminate()
    native.destroyContext(ctx)
    console.log(`mean ok: ${cases.length} cases`)
}

main(process.argv[2]).then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
