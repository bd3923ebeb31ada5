'use strict'
/**
 * GPU: power plane replies through the Node layer.  argv[2] is a directory pytest has filled (tests/test_node_power_gpu.py):
 * cases.json and, per case, the capture and the expected planes (raw f64, from tests/powerref.py).  Every case goes through
 * HipWorker.renderPower (asynchronous and synchronous, with and without `db`), the addon's renderPowerSync and `cli.js --power` /
 * `--power-db`; NaN positions must agree and every other value is compared bit for bit.  A peak detector is refused with status -4 and
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
    if (!got || got.width !== c.width || got.n !== c.n || !same(got.power, want)) throw new Error(`${what}: the plane differs`)
}

async function main(dir) {
    const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'))
    const worker = new HipWorker({ device: 0 })
    const ctx = native.createContext(0)
    for (const c of cases) {
        const file = path.join(dir, c.file)
        const bytes = fs.readFileSync(file)
        const buffer = bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
        const want = { power: f64(path.join(dir, c.id + '.power')), db: f64(path.join(dir, c.id + '.db')) }
        const w = native.window(c.window, c.n)
        const message = { buffer, format: c.format, n: c.n, windowc: Array.from(w.window), block_norm: 1.0 / w.weight, gain: c.gain,
            range: c.range, width: c.width, channelMode: c.channelMode, cmap: [[0, 0, 0], [255, 255, 255]], offset: 0 }
        check(`${c.id} renderPower`, await worker.renderPower(message), want.power, c)
        check(`${c.id} renderPower {db: false}`, await worker.renderPower(message, { db: false }), want.power, c)
        check(`${c.id} renderPower {db: true}`, await worker.renderPower(message, { db: true }), want.db, c)
        check(`${c.id} renderPowerSync (worker)`, worker.renderPowerSync(message), want.power, c)
        check(`${c.id} renderPowerSync (worker) {db: true}`, worker.renderPowerSync(message, { db: true }), want.db, c)
        const req = { format: native.parseFormat(c.format).id, buffer, n: c.n, width: c.width, windowc: w.window, block_norm: 1.0 / w.weight,
            gain: c.gain, range: c.range, channelMode: c.channelMode, db: false }
        check(`${c.id} renderPowerSync (addon)`, native.renderPowerSync(ctx, req), want.power, c)
        check(`${c.id} renderPowerSync (addon) db`, native.renderPowerSync(ctx, Object.assign({}, req, { db: true })), want.db, c)
        // cli.js --power / --power-db: raw little-endian f64 beside the image
        const outP = path.join(dir, c.id + '.power.out'), outD = path.join(dir, c.id + '.db.out'), img = path.join(dir, c.id + '.rgba')
        execFileSync(process.execPath, [path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js'), file, '--format', c.format, '--n',
            String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain), '--range', String(c.range), '--workers', '1',
            ...(c.channelMode ? ['--lr'] : []), '--power', outP, '--power-db', outD, '--out', img], { stdio: 'pipe' })
        if (fs.statSync(outP).size !== 8 * c.n * c.width || fs.statSync(outD).size !== 8 * c.n * c.width) throw new Error(`${c.id} cli: file size`)
        if (!same(f64(outP), want.power)) throw new Error(`${c.id} cli --power: the plane differs`)
        if (!same(f64(outD), want.db)) throw new Error(`${c.id} cli --power-db: the plane differs`)
        if (fs.statSync(img).size !== 4 * c.n * c.width) throw new Error(`${c.id} cli: image size`)

        // the two refusals: a peak detector -4, an unknown one -1, in onerror / a throw and never in an array
        for (const [detector, status] of [['peak', -4], ['rms', -1]]) {
            let events = 0, seen
            worker.onerror = (e) => { events++; seen = e.status }
            let got = null, err = null
            try { got = await worker.renderPower(Object.assign({}, message, { detector })) } catch (e) { err = e }
            await new Promise(r => setImmediate(r))
            worker.onerror = null
            if (got !== null || !err || err.status !== status || events !== 1 || seen !== status)
                throw new Error(`${c.id}: detector ${detector} was not refused with ${status} (${got}, ${err && err.status}, ${events}, ${seen})`)
            let thrown = null
            try { worker.renderPowerSync(Object.assign({}, message, { detector })) } catch (e) { thrown = e }
            if (!thrown || thrown.status !== status) throw new Error(`${c.id}: detector ${detector} (sync) was not refused with ${status}`)
        }
        let threw = false
        try { native.renderPowerSync(ctx, { format: 'cu8', buffer, n: c.n, width: c.width }) } catch (e) { threw = true }
        if (!threw) throw new Error('addon: a request without its numbers did not throw')
        check(`${c.id} after the refusals`, await worker.renderPower(message), want.power, c)
    }
    worker.terminate()
    native.destroyContext(ctx)
    console.log(`power ok: ${cases.length} cases`)
}

main(process.argv[2]).then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
