'use strict'
/**
 * GPU: indexed image replies through the Node layer.  argv[2] is a directory pytest has filled (tests/test_node_index_gpu.py):
 * cases.json and, per case, the capture, the colour map and the expected reply (index image and gauges raw, the rest as JSON with the
 * dBfs range as bit patterns).  Every case goes through HipWorker.renderIndexed, renderIndexedSync and the addon's renderIndexSync; the
 * whole reply is compared bit for bit, and recolour(index, cmap) with the RGBA image HipWorker.renderSync gives for the same message.
 * A malformed message ends in onerror with status -1 / a throw and never in an image.  `cli.js --index` writes a PGM whose payload
 * is the expected index image.
 */
const fs = require('fs')
const path = require('path')
const { execFileSync } = require('child_process')
const { HipWorker, recolour } = require('../../spectroplot-js_amd/js')
const native = require('../../spectroplot-js_amd/lib/spectroplot_hip.node')

function f64bits(v) { const b = Buffer.alloc(8); b.writeDoubleLE(v); return b.readBigUInt64LE().toString(16).padStart(16, '0') }
function sameBytes(a, b) { return Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0 }

function check(what, got, want, c) {
    if (!got || !(got.index instanceof Uint8Array) || !sameBytes(got.index, want.index)) throw new Error(`${what}: index differs`)
    if (got.width !== (c.waterfall ? c.n : c.width) || got.height !== (c.waterfall ? c.width : c.n)) throw new Error(`${what}: width / height`)
    for (const k of ['gauge_mins', 'gauge_maxs', 'gauge_amps'])
        if (!(got[k] instanceof Uint8ClampedArray) || !sameBytes(got[k], want[k])) throw new Error(`${what}: ${k} differs`)
    if (JSON.stringify(Array.from(got.c_hist)) !== JSON.stringify(want.c_hist)) throw new Error(`${what}: c_hist differs`)
    if (JSON.stringify(Array.from(got.cB_hist)) !== JSON.stringify(want.cB_hist)) throw new Error(`${what}: cB_hist differs`)
    if (f64bits(got.dBfs_min) !== want.dBfs_min || f64bits(got.dBfs_max) !== want.dBfs_max) throw new Error(`${what}: dBfs range differs`)
    const counts = new Array(want.c_hist.length).fill(0)
    for (let j = 0; j < got.index.length; j++) counts[got.index[j]]++
    if (JSON.stringify(counts) !== JSON.stringify(want.c_hist)) throw new Error(`${what}: bincount(index) != c_hist`)
}

async function main(dir) {
    const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'))
    const worker = new HipWorker({ device: 0 })
    const ctx = native.createContext(0)
    for (const c of cases) {
        const file = path.join(dir, c.file)
        const bytes = fs.readFileSync(file)
        const buffer = bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
        const lutBytes = fs.readFileSync(path.join(dir, c.id + '.lut'))
        const cmap = []
        for (let i = 0; i < lutBytes.length / 3; i++) cmap.push([lutBytes[3 * i], lutBytes[3 * i + 1], lutBytes[3 * i + 2]])
        const e = JSON.parse(fs.readFileSync(path.join(dir, c.id + '.json'), 'utf8'))
        const want = Object.assign(e, { index: new Uint8Array(fs.readFileSync(path.join(dir, c.id + '.index'))) })
        for (const k of ['gauge_mins', 'gauge_maxs', 'gauge_amps']) want[k] = new Uint8Array(fs.readFileSync(path.join(dir, c.id + '.' + k)))
        const w = native.window(c.window, c.n)
        const message = { buffer, format: c.format, n: c.n, windowc: Array.from(w.window), block_norm: 1.0 / w.weight, gain: c.gain,
            range: c.range, width: c.width, channelMode: c.channelMode, waterfall: c.waterfall, cmap, offset: 0, detector: c.detector }
        const got = await worker.renderIndexed(message)
        check(`${c.id} renderIndexed`, got, want, c)
        check(`${c.id} renderIndexedSync`, worker.renderIndexedSync(message), want, c)
        const req = { format: native.parseFormat(c.format).id, buffer, n: c.n, width: c.width, windowc: w.window, block_norm: 1.0 / w.weight,
            gain: c.gain, range: c.range, channelMode: c.channelMode, waterfall: c.waterfall, lut: new Uint8Array(lutBytes),
            detector: c.detector === 'peak' ? 1 : 0 }
        const raw = native.renderIndexSync(ctx, req)
        if (!sameBytes(raw.index, want.index)) throw new Error(`${c.id} renderIndexSync (addon): index differs`)
        // the postMessage path stays RGBA, and recolouring the index image gives that image
        const rgba = worker.renderSync(message).imageData.data
        if (!sameBytes(recolour(got.index, cmap), rgba)) throw new Error(`${c.id}: recolour(index, cmap) is not the RGBA reply`)

        // a malformed message: onerror with status -1 (and a throw from the synchronous form), never a different image
        const bad = [['detector', 'rms'], ['detector', 2], ['n', String(c.n)], ['width', '300'], ['gain', undefined], ['cmap', 'viridis'], ['buffer', 17]]
        for (const [k, v] of bad) {
            const events = []
            worker.onerror = ev => { events.push(ev) }
            let res = null, err = null
            try { res = await worker.renderIndexed(Object.assign({}, message, { [k]: v })) } catch (x) { err = x }
            await new Promise(r => setImmediate(r))
            worker.onerror = null
            if (res !== null || !err || events.length !== 1 || events[0].status !== -1)
                throw new Error(`${c.id}: ${k} = ${String(v)} did not end in onerror with status -1 (${res}, ${err}, ${JSON.stringify(events.map(x => x.status))})`)
            let threw = false
            try { worker.renderIndexedSync(Object.assign({}, message, { [k]: v })) } catch (x) { threw = true }
            if (!threw) throw new Error(`${c.id}: ${k} = ${String(v)} did not throw`)
        }
        for (const [k, v] of [['n', '256'], ['width', 1.5], ['range', 'wide'], ['windowc', new Float64Array(3)], ['lut', 'x'], ['detector', 7]]) {
            let threw = false
            try { native.renderIndexSync(ctx, Object.assign({}, req, { [k]: v })) } catch (x) { threw = true }
            if (!threw) throw new Error(`${c.id} addon: ${k} = ${String(v)} did not throw`)
        }
        check(`${c.id} after the errors`, await worker.renderIndexed(message), want, c)

        // cli.js --index: a binary PGM beside the image (sample detector or peak, by name)
        if (c.cli) {
            const pgm = path.join(dir, c.id + '.pgm'), img = path.join(dir, c.id + '.rgba')
            execFileSync(process.execPath, [path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js'), file, '--format', c.format, '--n',
                String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain), '--range', String(c.range), '--workers', '1',
                ...(c.channelMode ? ['--lr'] : []), ...(c.waterfall ? ['--waterfall'] : []), ...(c.detector ? ['--detector', c.detector] : []),
                '--index', pgm, '--out', img], { stdio: 'pipe' })
            const out = fs.readFileSync(pgm)
            const header = `P5\n${c.waterfall ? c.n : c.width} ${c.waterfall ? c.width : c.n}\n255\n`
            if (out.slice(0, header.length).toString() !== header) throw new Error(`${c.id} cli: PGM header`)
            if (Buffer.compare(out.slice(header.length), Buffer.from(want.index)) !== 0) throw new Error(`${c.id} cli: PGM payload differs`)
            if (fs.statSync(img).size !== 4 * c.n * c.width) throw new Error(`${c.id} cli: image size`)
        }
    }
    worker.terminate()
    native.destroyContext(ctx)
    console.log(`index ok: ${cases.length} cases`)
}

main(process.argv[2]).then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
