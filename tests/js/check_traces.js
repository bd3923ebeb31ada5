'use strict'
/**
 * GPU: per-bin min / max traces through the Node layer.  argv[2] is a directory pytest has filled (tests/test_node_traces_gpu.py):
 * cases.json and, per case, the capture and the expected arrays (raw f64, from tests/tracesref.py).  Every case goes through
 * HipWorker.renderTraces, the addon's renderTracesSync and `cli.js --traces`; both arrays are compared bit for bit.  A malformed field
 * ends in onerror / a throw and never in arrays.
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
    for (let i = 0; i < x.length; i++) if (x[i] !== y[i]) return false
    return true
}
function f64(file) {
    const b = fs.readFileSync(file)
    return new Float64Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength))
}
function check(what, got, want) {
    if (!got || !same(got.trace_min, want.trace_min) || !same(got.trace_max, want.trace_max)) throw new Error(`${what}: traces differ`)
}

async function main(dir) {
    const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'))
    const worker = new HipWorker({ device: 0 })
    const ctx = native.createContext(0)
    let last = null
    for (const c of cases) {
        const file = path.join(dir, c.file)
        const bytes = fs.readFileSync(file)
        const buffer = bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
        const want = { trace_min: f64(path.join(dir, c.id + '.tmin')), trace_max: f64(path.join(dir, c.id + '.tmax')) }
        const w = native.window(c.window, c.n)
        const message = { buffer, format: c.format, n: c.n, windowc: Array.from(w.window), block_norm: 1.0 / w.weight, gain: c.gain,
            range: c.range, width: c.width, channelMode: c.channelMode, cmap: [[0, 0, 0], [255, 255, 255]], offset: 0 }
        check(`${c.id} renderTraces`, await worker.renderTraces(message), want)
        check(`${c.id} renderTracesSync (worker)`, worker.renderTracesSync(message), want)
        const req = { format: native.parseFormat(c.format).id, buffer, n: c.n, width: c.width, windowc: w.window, block_norm: 1.0 / w.weight,
            gain: c.gain, range: c.range, channelMode: c.channelMode }
        check(`${c.id} renderTracesSync (addon)`, native.renderTracesSync(ctx, req), want)
        last = { id: c.id, req, want }
        // cli.js --traces: JSON beside the image
        const out = path.join(dir, c.id + '.json.out'), img = path.join(dir, c.id + '.rgba')
        execFileSync(process.execPath, [path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js'), file, '--format', c.format, '--n',
            String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain), '--range', String(c.range), '--workers', '1',
            ...(c.channelMode ? ['--lr'] : []), '--traces', out, '--out', img], { stdio: 'pipe' })
        const j = JSON.parse(fs.readFileSync(out, 'utf8'))
        if (j.n !== c.n || j.width !== c.width) throw new Error(`${c.id} cli: header`)
        check(`${c.id} cli`, { trace_min: Float64Array.from(j.trace_min, Number), trace_max: Float64Array.from(j.trace_max, Number) }, want)
        if (fs.statSync(img).size !== 4 * c.n * c.width) throw new Error(`${c.id} cli: image size`)

        // malformed fields: onerror / a throw, never arrays
        const bad = [['n', 'x'], ['width', 1.5], ['width', -1], ['gain', undefined], ['range', 'wide'], ['block_norm', null], ['windowc', [1, 2, 3]],
            ['detector', 'peak'], ['detector', 'rms'], ['buffer', 17]]
        for (const [k, v] of bad) {
            let events = 0
            worker.onerror = () => { events++ }
            let got = null, err = null
            try { got = await worker.renderTraces(Object.assign({}, message, { [k]: v })) } catch (e) { err = e }
            await new Promise(r => setImmediate(r))
            worker.onerror = null
            if (got !== null || !err || events !== 1) throw new Error(`${c.id}: ${k} = ${String(v)} did not end in onerror (${got}, ${err}, ${events})`)
            let threw = false
            try { worker.renderTracesSync(Object.assign({}, message, { [k]: v })) } catch (e) { threw = true }
            if (!threw) throw new Error(`${c.id}: ${k} = ${String(v)} did not throw`)
        }
        let threw = false
        try { native.renderTracesSync(ctx, { format: 'cu8', buffer, n: c.n, width: c.width }) } catch (e) { threw = true }
        if (!threw) throw new Error('addon: a request without its numbers did not throw')
        check(`${c.id} after the errors`, await worker.renderTraces(message), want)
    }
    // the job lifecycle the addon shares between its request kinds: while a traces request is in flight on a handle, a second one is
    // refused; a handle destroyed before the callback still delivers the traces, and is released once the request has returned
    {
        const h = native.createContext(0)
        const done = new Promise((resolve, reject) => native.renderTraces(h, last.req, (err, r) => err ? reject(err) : resolve(r)))
        let called = false
        for (const [what, f] of [['renderTraces', () => native.renderTraces(h, last.req, () => { called = true })],
                                 ['renderTracesSync', () => native.renderTracesSync(h, last.req)]]) {
            let msg = ''
            try { f() } catch (e) { msg = e.message }
            if (msg !== 'a render is already in flight on this context') throw new Error(`${what} during a request in flight: "${msg}"`)
        }
        if (native.destroyContext(h) !== false) throw new Error('destroyContext released a context with a request in flight')
        check(`${last.id} renderTraces (addon) after destroyContext`, await done, last.want)
        await new Promise(r => setImmediate(r))
        if (called) throw new Error('a refused request called back')
        let msg = ''
        try { native.renderTracesSync(h, last.req) } catch (e) { msg = e.message }
        if (!/destroyed/.test(msg)) throw new Error(`a destroyed handle took a request: "${msg}"`)
    }
    worker.terminate()
    native.destroyContext(ctx)
    console.log(`traces ok: ${cases.length} cases`)
}

main(process.argv[2]).then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
