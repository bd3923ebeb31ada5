'use strict'
/**
 * GPU: the persistence spectrum through the Node layer.  argv[2] is a directory pytest has filled (tests/test_node_density_gpu.py):
 * cases.json and, per case, the capture, the colour map, the expected counts (little-endian uint32, n rows of lutLen) and the body of
 * the PGM `cli.js --density` must write (big-endian uint16, saturated at 65535).  Every case goes through HipWorker.renderDensity,
 * renderDensitySync and the addon's renderDensitySync, compared bit for bit.  A malformed message ends in onerror with status -1 (a
 * colour map of 257 entries: -4) / a throw and never in counts.
 */
const fs = require('fs')
const path = require('path')
const { execFileSync } = require('child_process')
const { HipWorker } = require('../../spectroplot-js_amd/js')
const native = require('../../spectroplot-js_amd/lib/spectroplot_hip.node')

function sameBytes(a, b) { return Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0 }

function check(what, got, want, c, lutLen) {
    if (!got || !(got.density instanceof Uint32Array) || got.density.length !== c.n * lutLen) throw new Error(`${what}: no Uint32Array(n * lutLen)`)
    if (got.n !== c.n || got.lutLen !== lutLen || got.width !== c.width) throw new Error(`${what}: n / lutLen / width`)
    if (!sameBytes(got.density, want)) throw new Error(`${what}: counts differ`)
    for (let y = 0; y < c.n; y++) {
        let sum = 0
        for (let g = 0; g < lutLen; g++) sum += got.density[y * lutLen + g]
        if (sum !== c.width) throw new Error(`${what}: row ${y} sums to ${sum}, not to the width`)
    }
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
        const lutLen = cmap.length
        const raw = fs.readFileSync(path.join(dir, c.id + '.density'))
        const want = new Uint32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength))
        const w = native.window(c.window, c.n)
        const message = { buffer, format: c.format, n: c.n, windowc: Array.from(w.window), block_norm: 1.0 / w.weight, gain: c.gain,
            range: c.range, width: c.width, channelMode: c.channelMode, waterfall: c.waterfall, cmap, offset: 0, detector: c.detector }
        check(`${c.id} renderDensity`, await worker.renderDensity(message), want, c, lutLen)
        check(`${c.id} renderDensitySync`, worker.renderDensitySync(message), want, c, lutLen)
        const req = { format: native.parseFormat(c.format).id, buffer, n: c.n, width: c.width, windowc: w.window, block_norm: 1.0 / w.weight,
            gain: c.gain, range: c.range, channelMode: c.channelMode, waterfall: c.waterfall, lut: new Uint8Array(lutBytes),
            detector: c.detector === 'peak' ? 1 : 0 }
        check(`${c.id} renderDensitySync (addon)`, native.renderDensitySync(ctx, req), want, c, lutLen)

        // a malformed message: onerror with its status (and a throw from the synchronous form), never counts
        const long = []
        for (let i = 0; i < 257; i++) long.push([i & 255, i >> 8, 0])
        const bad = [['n', '64', -1], ['cmap', undefined, -1], ['detector', 'rms', -1], ['cmap', long, -4], ['width', '300', -1], ['buffer', 17, -1]]
        for (const [k, v, status] of bad) {
            const events = []
            worker.onerror = ev => { events.push(ev) }
            let res = null, err = null
            try { res = await worker.renderDensity(Object.assign({}, message, { [k]: v })) } catch (x) { err = x }
            await new Promise(r => setImmediate(r))
            worker.onerror = null
            if (res !== null || !err || events.length !== 1 || events[0].status !== status)
                throw new Error(`${c.id}: ${k} = ${String(v).slice(0, 20)} did not end in onerror with status ${status} (${res}, ${err}, ${JSON.stringify(events.map(x => x.status))})`)
            let threw = null
            try { worker.renderDensitySync(Object.assign({}, message, { [k]: v })) } catch (x) { threw = x }
            if (!threw) throw new Error(`${c.id}: ${k} = ${String(v).slice(0, 20)} did not throw`)
        }
        for (const [k, v] of [['n', '256'], ['width', 1.5], ['range', 'wide'], ['windowc', new Float64Array(3)], ['lut', 'x'], ['detector', 7]]) {
            let threw = false
            try { native.renderDensitySync(ctx, Object.assign({}, req, { [k]: v })) } catch (x) { threw = true }
            if (!threw) throw new Error(`${c.id} addon: ${k} = ${String(v)} did not throw`)
        }
        let status = null
        try { native.renderDensitySync(ctx, Object.assign({}, req, { lut: new Uint8Array(3 * 257) })) } catch (x) { status = x.status }
        if (status !== -4) throw new Error(`${c.id} addon: a 257-entry colour map gave status ${status}, not -4`)
        check(`${c.id} after the errors`, await worker.renderDensity(message), want, c, lutLen)

        // cli.js --density: a binary PGM of lutLen columns x n rows, maxval 65535, big-endian, saturated counts
        if (c.cli) {
            const pgm = path.join(dir, c.id + '.pgm'), img = path.join(dir, c.id + '.rgba')
            execFileSync(process.execPath, [path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js'), file, '--format', c.format, '--n',
                String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain), '--range', String(c.range), '--workers', '1',
                ...(c.channelMode ? ['--lr'] : []), ...(c.waterfall ? ['--waterfall'] : []), ...(c.detector ? ['--detector', c.detector] : []),
                '--density', pgm, '--out', img], { stdio: 'pipe' })
            const out = fs.readFileSync(pgm)
            const header = `P5\n${lutLen} ${c.n}\n65535\n`
            if (out.slice(0, header.length).toString() !== header) throw new Error(`${c.id} cli: PGM header`)
            if (Buffer.compare(out.slice(header.length), fs.readFileSync(path.join(dir, c.id + '.pgm_body'))) !== 0) throw new Error(`${c.id} cli: PGM payload differs`)
        }
    }
    worker.terminate()
    native.destroyContext(ctx)
    console.log(`density ok: ${cases.length} cases`)
}

main(process.argv[2]).then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
