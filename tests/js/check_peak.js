'use strict'
/**
 * GPU: the peak detector through the Node layer.  argv[2] is a directory pytest has filled (tests/test_node_peak_gpu.py): cases.json and,
 * per case, the capture and the expected reply built from the oracle (tests/peakref.py).  Every case is rendered through
 * HipWorker.postMessage (evaluated arrays), HipWorker.renderNamed, renderSliced with two workers (each slice its own request, compared
 * with per-slice expectations) and `cli.js --detector peak`; every reply field is compared.  An unknown detector ends in onerror with
 * status -1 and never in an image; `device: true` and batches refuse the peak detector.
 */
const fs = require('fs')
const path = require('path')
const { execFileSync } = require('child_process')
const { HipWorker, renderSliced, renderMany, cmapByName } = require('../../spectroplot-js_amd/js')
const native = require('../../spectroplot-js_amd/lib/spectroplot_hip.node')

function same(a, b) {
    if (a.length !== b.length) return false
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false
    return true
}

function load(dir, c, tag) {
    const bin = name => new Uint8Array(fs.readFileSync(path.join(dir, `${c.id}${tag}.${name}`)))
    const j = JSON.parse(fs.readFileSync(path.join(dir, `${c.id}${tag}.json`), 'utf8'))
    j.dBfs_min = Number(j.dBfs_min); j.dBfs_max = Number(j.dBfs_max)   // (strings: JSON has no infinities)
    return Object.assign({ rgba: bin('rgba'), gauge_mins: bin('gmin'), gauge_maxs: bin('gmax'), gauge_amps: bin('gamp') }, j)
}

function diff(reply, want) {
    const bad = []
    if (!same(reply.imageData.data, want.rgba)) bad.push('imageData')
    for (const k of ['gauge_mins', 'gauge_maxs', 'gauge_amps']) if (!same(reply[k], want[k])) bad.push(k)
    for (const k of ['c_hist', 'cB_hist']) if (!same(reply[k], want[k])) bad.push(k)
    if (!Object.is(reply.dBfs_min, want.dBfs_min) || !Object.is(reply.dBfs_max, want.dBfs_max)) bad.push('dBfs range')
    return bad
}

function post(worker, message) {
    return new Promise((resolve, reject) => {
        worker.onmessage = e => resolve(e.data)
        worker.onerror = e => reject(Object.assign(new Error(e.message), { status: e.status }))
        worker.postMessage(message, [message.buffer])
    })
}

async function main() {
    const dir = process.argv[2]
    const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'))
    const failures = []
    const worker = new HipWorker({ device: 0 })
    const cli = path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js')
    for (const c of cases) {
        const file = path.join(dir, c.file)
        const bytes = fs.readFileSync(file)
        const buffer = () => bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
        const want = load(dir, c, '')
        const m = HipWorker.peakSubframes(c.format, c.n, bytes.length, c.width)
        if (m.subframes !== c.M || m.lastColumnCount !== c.last) failures.push(`${c.id}: peakSubframes ${JSON.stringify(m)}`)
        const w = native.window(c.window, c.n)
        const cmap = cmapByName(c.cmap).map(x => x.slice())
        cmap[0] = [0, 0, 0]; cmap[cmap.length - 1] = [255, 255, 255]
        const message = { block_norm: 1.0 / w.weight, gain: c.gain, range: c.range, cmap, n: c.n, windowc: w.window, width: c.width, offset: 0,
            buffer: buffer(), format: c.format, channelMode: c.channelMode, waterfall: c.waterfall, detector: 'peak' }
        let bad = diff(await post(worker, message), want)
        if (bad.length) failures.push(`${c.id}: postMessage differs in ${bad}`)
        const named = { buffer: buffer(), format: c.format, window: c.window, cmap: c.cmap, n: c.n, width: c.width, gain: c.gain, range: c.range,
            channelMode: c.channelMode, waterfall: c.waterfall, detector: 'peak' }
        bad = diff(await worker.renderNamed(named), want)
        if (bad.length) failures.push(`${c.id}: renderNamed differs in ${bad}`)
        // 'sample' and an absent detector are the reference: the same reply, which is not the peak reply
        const plain = await worker.renderNamed(Object.assign({}, named, { buffer: buffer(), detector: undefined }))
        const sample = await worker.renderNamed(Object.assign({}, named, { buffer: buffer(), detector: 'sample' }))
        if (diff(sample, { rgba: plain.imageData.data, gauge_mins: plain.gauge_mins, gauge_maxs: plain.gauge_maxs, gauge_amps: plain.gauge_amps,
            c_hist: plain.c_hist, cB_hist: plain.cB_hist, dBfs_min: plain.dBfs_min, dBfs_max: plain.dBfs_max }).length) failures.push(`${c.id}: 'sample' is not the default`)
        if (c.M >= 2 && same(plain.imageData.data, want.rgba)) failures.push(`${c.id}: the peak expectation equals the sample image (nothing is tested)`)
        // two workers: each slice is its own request with its own stride and M
        const two = await renderSliced({ buffer: buffer(), format: c.format, n: c.n, width: c.width, workers: 2, byName: true, window: c.window,
            cmap: c.cmap, gain: c.gain, range: c.range, channelMode: c.channelMode, waterfall: c.waterfall, detector: 'peak' })
        for (let k = 0; k < 2; k++) {
            bad = diff(two.replies[k], load(dir, c, `.s${k}`))
            if (bad.length) failures.push(`${c.id}: renderSliced slice ${k} differs in ${bad}`)
        }
        // the command line
        const out = path.join(dir, `${c.id}.cli.rgba`)
        const args = [cli, file, '--format', c.format, '--n', String(c.n), '--width', String(c.width), '--window', c.window, '--cmap', c.cmap,
            '--gain', String(c.gain), '--range', String(c.range), '--workers', '1', '--detector', 'peak', '--out', out]
        if (c.waterfall) args.push('--waterfall')
        if (c.channelMode) args.push('--lr')
        execFileSync('node', args)
        if (!same(new Uint8Array(fs.readFileSync(out)), want.rgba)) failures.push(`${c.id}: cli.js --detector peak differs`)
        let refused = false
        try { execFileSync('node', args.map(a => a === 'peak' ? 'rms' : a), { stdio: 'pipe' }) } catch (e) { refused = e.status === 1 }
        if (!refused) failures.push(`${c.id}: cli.js --detector rms did not fail`)

        // anything else: onerror with status -1, never an image
        for (const d of ['rms', 'PEAK', 1, true, {}]) {
            let got = null, err = null
            try { got = await post(worker, Object.assign({}, message, { buffer: buffer(), detector: d })) } catch (e) { err = e }
            if (got || !err || err.status !== -1) failures.push(`${c.id}: detector ${JSON.stringify(d)} on a message: ${got ? 'an image' : err && err.status}`)
            got = null; err = null
            try { got = await worker.renderNamed(Object.assign({}, named, { buffer: buffer(), detector: d })) } catch (e) { err = e }
            if (got || !err || err.status !== -1) failures.push(`${c.id}: detector ${JSON.stringify(d)} on renderNamed: ${got ? 'an image' : err && err.status}`)
        }
        // the addon itself checks what it is handed (no stale or coerced value)
        for (const d of ['peak', 2, 0.5, null]) {
            let threw = false
            try { native.renderNamedSync(worker._ctx, Object.assign(worker._namedRequest(named), { buffer: buffer(), detector: d })) } catch (e) { threw = true }
            if (!threw) failures.push(`${c.id}: the addon accepted detector ${JSON.stringify(d)}`)
        }
        // groups and batches refuse
        for (const [what, run] of [['device: true', () => renderSliced({ buffer: buffer(), format: c.format, n: c.n, width: c.width, workers: 1,
            window: c.window, cmap, gain: c.gain, range: c.range, device: true, detector: 'peak' })],
        ['renderMany', () => renderMany({ buffers: [buffer()], format: c.format, n: c.n, width: c.width, window: c.window, cmap, detector: 'peak' })]]) {
            let err = null
            try { await run() } catch (e) { err = e }
            if (!err || err.status !== -4) failures.push(`${c.id}: ${what} with the peak detector: ${err ? err.status : 'rendered'}`)
        }
    }
    // the library's own refusal behind the addon's batch entry
    {
        const c = cases[0]
        const w = native.window(c.window, c.n)
        const h = native.createContext(0)
        let err = null
        try {
            native.renderBatchSync(h, { format: native.parseFormat(c.format).id, n: c.n, windowc: w.window, block_norm: 1 / w.weight, gain: 3, range: 40,
                lut: new Uint8Array(3 * 256), channelMode: false, waterfall: false, detector: 1 }, [{ buffer: new ArrayBuffer(4096), width: 4 }])
        } catch (e) { err = e }
        native.destroyContext(h)
        if (!err || err.status !== -4) failures.push(`addon.renderBatchSync with detector 1: ${err ? err.status : 'rendered'}`)
    }
    worker.terminate()
    if (failures.length) { console.log(failures.join('\n')); process.exit(1) }
    console.log('peak ok: ' + cases.length + ' cases')
    process.exit(0)
}

main().catch(e => { console.error(e); process.exit(1) })
