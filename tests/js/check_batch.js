'use strict'
/**
 * GPU: batches from Node (renderMany -> addon.renderBatch -> sp_render_batch) and the command-line renderer's --out-dir mode.
 *   - renderMany equals renderSliced (evaluated arrays, one worker) per buffer, byte for byte: image, histograms, dBfs range;
 *   - cli.js a b c --out-dir DIR writes the same bytes as single-file cli.js runs on the same captures;
 *   - a malformed item (a width that is not a number, a missing buffer) raises an error and never returns an image.
 */
const fs = require('fs')
const os = require('os')
const path = require('path')
const { execFileSync } = require('child_process')
const { renderSliced, renderMany, cmapByName } = require('../../spectroplot-js_amd/js')

function capture(bytes, seed) {
    const b = new Uint8Array(bytes)
    let x = seed >>> 0
    for (let i = 0; i < bytes; i++) { x = (Math.imul(x, 1664525) + 1013904223) >>> 0; b[i] = (x >>> 24) ^ ((i * 37) & 255) }
    return b.buffer
}

function same(a, b) {
    if (a.length !== b.length) return false
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false
    return true
}

async function main() {
    const failures = []
    const cmap = cmapByName('viridis')
    const shapes = [[4096, 64], [9000, 257], [100, 5], [20000, 33], [2048, 0], [65536, 512]]
    for (const [fmt, n] of [['cu8', 256], ['cs16', 512], ['cf32', 128], ['cu8', 2048]]) {
        const buffers = shapes.map(([bytes], k) => capture(bytes - bytes % 8, 7 * k + n))
        const widths = shapes.map(([, w]) => w)
        const opts = { format: fmt, n, window: 'hann', cmap, gain: 3, range: 40, waterfall: n === 512 }
        const many = await renderMany(Object.assign({ buffers, widths }, opts))
        for (let k = 0; k < buffers.length; k++) {
            const one = await renderSliced(Object.assign({ buffer: buffers[k].slice(0), width: widths[k], workers: 1 }, opts))
            const m = many[k]
            const ok = same(m.data, one.data) && same(m.c_hist, one.c_hist) && same(m.cB_hist, one.cB_hist)
                && Object.is(m.dBfs_min, one.dBfs_min) && Object.is(m.dBfs_max, one.dBfs_max) && m.width === one.width && m.height === one.height
            if (!ok) failures.push(`renderMany ${fmt} n=${n} item ${k} differs from renderSliced`)
        }
    }

    const dir = fs.mkdtempSync(path.join(os.tmpdir(), 'sp_batch_'))
    const cli = path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js')
    const files = [['a_433.92M_250k.cu8', 300000], ['b_433.92M_250k.cu8', 77777 * 2], ['c_868M_1000k.cs16', 400000], ['d.cu8', 999]]
        .map(([name, bytes], k) => { const f = path.join(dir, name); fs.writeFileSync(f, Buffer.from(capture(bytes, 100 + k))); return f })
    const common = ['--n', '256', '--width', '300', '--window', 'hamming', '--cmap', 'magma', '--gain', '2', '--range', '45']
    execFileSync('node', [cli, ...files, ...common, '--out-dir', path.join(dir, 'out')])
    for (const f of files) {
        const single = path.join(dir, path.basename(f) + '.single.ppm')
        execFileSync('node', [cli, f, ...common, '--workers', '1', '--out', single])
        const a = fs.readFileSync(single), b = fs.readFileSync(path.join(dir, 'out', path.basename(f) + '.ppm'))
        if (!a.equals(b)) failures.push(`cli --out-dir: ${path.basename(f)} differs from the single-file run`)
    }
    fs.rmSync ? fs.rmSync(dir, { recursive: true, force: true }) : null

    for (const [what, o] of [['non-numeric width', { buffers: [capture(4096, 1)], widths: ['12'] }],
                             ['missing buffer', { buffers: [undefined], widths: [12] }],
                             ['fractional width', { buffers: [capture(4096, 1)], widths: [1.5] }]]) {
        let got = null, threw = false
        try { got = await renderMany(Object.assign({ format: 'cu8', n: 256, cmap }, o)) } catch (e) { threw = true }
        if (!threw || got) failures.push(`renderMany accepted a malformed item: ${what}`)
    }
    const native = require('../../spectroplot-js_amd/lib/spectroplot_hip.node')
    const h = native.createContext(0)
    const req = { format: 2, n: 256, windowc: new Float64Array(256).fill(1), block_norm: 1 / 256, gain: 0, range: 30, lut: new Uint8Array(768),
        channelMode: false, waterfall: false }
    for (const [what, items] of [['width string', [{ buffer: capture(4096, 2), width: 'x' }]], ['no buffer', [{ width: 4 }]],
                                 ['not an array', { buffer: capture(64, 3), width: 1 }]]) {
        let threw = false, got = null
        try { got = native.renderBatchSync(h, req, items) } catch (e) { threw = true }
        if (!threw || got) failures.push(`renderBatchSync accepted ${what}`)
    }
    // the job lifecycle the addon shares between its request kinds: while a batch is in flight on a handle, a second one is refused;
    // a handle destroyed before the callback still delivers the batch, and is released once the batch has returned
    {
        const items = [{ buffer: capture(65536, 5), width: 200 }, { buffer: capture(9000, 6), width: 33 }, { buffer: capture(2048, 7), width: 0 }]
        const want = native.renderBatchSync(h, req, items)
        const h2 = native.createContext(0)
        const done = new Promise((resolve, reject) => native.renderBatch(h2, req, items, (err, r) => err ? reject(err) : resolve(r)))
        for (const [what, f] of [['renderBatch', () => native.renderBatch(h2, req, items, () => failures.push('a refused batch called back'))],
                                 ['renderBatchSync', () => native.renderBatchSync(h2, req, items)]]) {
            let msg = ''
            try { f() } catch (e) { msg = e.message }
            if (msg !== 'a render is already in flight on this context') failures.push(`${what} during a batch in flight: "${msg}"`)
        }
        if (native.destroyContext(h2) !== false) failures.push('destroyContext released a context with a batch in flight')
        const got = await done
        const bytes = (x) => new Uint8Array(x.buffer || x, x.byteOffset || 0, x.byteLength)
        if (!Array.isArray(got) || got.length !== want.length) failures.push('renderBatch after destroyContext: no replies')
        else for (let k = 0; k < want.length; k++) {
            for (const f of ['rgba', 'gauge_mins', 'gauge_maxs', 'gauge_amps', 'c_hist', 'cB_hist'])
                if (!same(bytes(got[k][f]), bytes(want[k][f]))) failures.push(`renderBatch after destroyContext: item ${k} ${f} differs`)
            if (!Object.is(got[k].dBfs_min, want[k].dBfs_min) || !Object.is(got[k].dBfs_max, want[k].dBfs_max))
                failures.push(`renderBatch after destroyContext: item ${k} dBfs range differs`)
        }
        if (want[0].rgba.byteLength !== 4 * 200 * 256 || !bytes(want[0].rgba).some(v => v !== 0)) failures.push('the lifecycle batch renders nothing')
        let msg = ''
        try { native.renderBatchSync(h2, req, items) } catch (e) { msg = e.message }
        if (!/destroyed/.test(msg)) failures.push(`a destroyed handle took a batch: "${msg}"`)
    }
    native.destroyContext(h)

    if (failures.length) { console.log(failures.join('\n')); process.exit(1) }
    console.log('batch ok: renderMany = renderSliced per buffer, cli --out-dir = single-file runs, malformed items refused')
}

main().then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
