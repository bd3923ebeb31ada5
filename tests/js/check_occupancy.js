'use strict'
/**
 * GPU: the occupancy counts through the Node layer.  argv[2] is a directory pytest has filled (tests/test_node_occupancy_gpu.py):
 * cases.json and, per case, the capture, a threshold per row (raw f64) and the expected counts (raw uint32: n rows, count * width frames,
 * band-major, from tests/occref.py) for that threshold, for K times the mean trace (.k) and for one power for all rows (.p).  Every case
 * goes through HipWorker.renderOccupancy (asynchronous and synchronous, a Float64Array and a number), the addon's renderOccupancy /
 * renderOccupancySync and `cli.js --occupancy-rows` / `--occupancy-frames` with --threshold and --threshold-over-mean; every word must be
 * equal.  A peak detector is refused with status -4, bad bands and a threshold of the wrong length with -1, before anything is rendered.
 */
const fs = require('fs')
const path = require('path')
const { execFileSync } = require('child_process')
const { HipWorker } = require('../../spectroplot-js_amd/js')
const native = require('../../spectroplot-js_amd/lib/spectroplot_hip.node')

function sameWords(a, b) {
    if (!(a instanceof Uint32Array) || a.length !== b.length) return false
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false
    return true
}
function read(file, Type) {
    const b = fs.readFileSync(file)
    return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength))
}
function check(what, got, want, c, count) {
    if (!got || got.width !== c.width || got.n !== c.n || got.count !== count || want.rows.length !== c.n || !sameWords(got.rows, want.rows))
        throw new Error(`${what}: the row counts differ`)
    if (want.frames.length < count * c.width || !sameWords(got.frames, want.frames.subarray(0, count * c.width)))
        throw new Error(`${what}: the frame counts differ`)
}

async function main(dir) {
    const cases = JSON.parse(fs.readFileSync(path.join(dir, 'cases.json'), 'utf8'))
    const worker = new HipWorker({ device: 0 })
    const ctx = native.createContext(0)
    const cli = path.join(__dirname, '..', '..', 'spectroplot-js_amd', 'js', 'cli.js')
    for (const c of cases) {
        const file = path.join(dir, c.file)
        const bytes = fs.readFileSync(file)
        const buffer = bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength)
        const wants = {}
        for (const tag of ['', '.k', '.p'])
            wants[tag] = { rows: read(path.join(dir, c.id + tag + '.rows'), Uint32Array), frames: read(path.join(dir, c.id + tag + '.frames'), Uint32Array) }
        const want = wants[''], threshold = read(path.join(dir, c.id + '.thr'), Float64Array)
        const bands = c.rows.concat(c.rowsOfFreqs), count = bands.length
        const w = native.window(c.window, c.n)
        const message = { buffer, format: c.format, n: c.n, windowc: Array.from(w.window), block_norm: 1.0 / w.weight, gain: c.gain,
            range: c.range, width: c.width, channelMode: c.channelMode, cmap: [[0, 0, 0], [255, 255, 255]], offset: 0 }
        check(`${c.id} renderOccupancy`, await worker.renderOccupancy(message, { threshold, bands }), want, c, count)
        check(`${c.id} renderOccupancy (flat Int32Array)`,
            await worker.renderOccupancy(message, { threshold, bands: Int32Array.from([].concat(...bands)) }), want, c, count)
        check(`${c.id} renderOccupancy (a number)`, await worker.renderOccupancy(message, { threshold: c.power, bands }), wants['.p'], c, count)
        check(`${c.id} renderOccupancy (no bands)`, await worker.renderOccupancy(message, { threshold }), want, c, 0)
        check(`${c.id} renderOccupancySync (worker)`, worker.renderOccupancySync(message, { threshold, bands }), want, c, count)
        const req = { format: native.parseFormat(c.format).id, buffer, n: c.n, width: c.width, windowc: w.window, block_norm: 1.0 / w.weight,
            gain: c.gain, range: c.range, channelMode: c.channelMode, threshold, bands: Int32Array.from([].concat(...bands)) }
        check(`${c.id} renderOccupancySync (addon)`, native.renderOccupancySync(ctx, req), want, c, count)
        const viaCallback = await new Promise((resolve, reject) => native.renderOccupancy(ctx, req, (err, r) => err ? reject(err) : resolve(r)))
        check(`${c.id} renderOccupancy (addon)`, viaCallback, want, c, count)
        const none = native.renderOccupancySync(ctx, Object.assign({}, req, { bands: new Int32Array(0) }))
        if (none.count !== 0 || none.frames.length !== 0 || !sameWords(none.rows, want.rows)) throw new Error(`${c.id}: no bands did not give the rows alone`)
        // K times the mean trace by hand: what cli.js --threshold-over-mean does
        const mean = (await worker.renderMean(message)).mean
        check(`${c.id} K * renderMean`, await worker.renderOccupancy(message, { threshold: mean.map(v => c.overMean * v), bands }), wants['.k'], c, count)
        // the addon hands the library's refusal on: status -1 for bands it does not take and for a threshold of another length
        for (const own of [{ bands: Int32Array.from([0, c.n + 1]) }, { bands: Int32Array.from([4, 3]) }, { bands: Int32Array.from([-1, 2]) },
            { bands: new Int32Array(130) }, { threshold: threshold.subarray(1) }, { threshold: new Float64Array(0) }]) {
            let thrown = null
            try { native.renderOccupancySync(ctx, Object.assign({}, req, own)) } catch (e) { thrown = e }
            if (!thrown || thrown.status !== -1) throw new Error(`${c.id} addon: ${Object.keys(own)} was not refused with -1`)
        }
        for (const own of [{ bands: Int32Array.from([0, 1, 2]) }, { bands: undefined }, { threshold: undefined }, { threshold: Array.from(threshold) },
            { threshold: Float32Array.from(threshold) }]) {
            let threw = false
            try { native.renderOccupancySync(ctx, Object.assign({}, req, own)) } catch (e) { threw = true }
            if (!threw) throw new Error(`${c.id} addon: a malformed ${Object.keys(own)} did not throw`)
        }

        // cli.js --occupancy-rows / --occupancy-frames: raw little-endian uint32; --bands first, then --band-freqs
        const outR = path.join(dir, c.id + '.rows.out'), outF = path.join(dir, c.id + '.frames.out'), img = path.join(dir, c.id + '.rgba')
        const common = [cli, file, '--format', c.format, '--n', String(c.n), '--width', String(c.width), '--window', c.window, '--gain', String(c.gain),
            '--range', String(c.range), '--workers', '1', ...(c.channelMode ? ['--lr'] : []), '--out', img]
        const bandArgs = ['--bands', c.rows.map(r => r.join(':')).join(','), '--band-freqs', c.freqs.map(r => r.join(':')).join(',')]
        for (const [tag, args] of [['.k', ['--threshold-over-mean', String(c.overMean)]], ['.p', ['--threshold', String(c.power)]]]) {
            for (const f of [outR, outF]) if (fs.existsSync(f)) fs.unlinkSync(f)
            execFileSync(process.execPath, [...common, ...bandArgs, ...args, '--occupancy-rows', outR, '--occupancy-frames', outF], { stdio: 'pipe' })
            if (fs.statSync(outR).size !== 4 * c.n || fs.statSync(outF).size !== 4 * count * c.width) throw new Error(`${c.id} cli ${args[0]}: file size`)
            if (!sameWords(read(outR, Uint32Array), wants[tag].rows)) throw new Error(`${c.id} cli ${args[0]} --occupancy-rows: the counts differ`)
            if (!sameWords(read(outF, Uint32Array), wants[tag].frames)) throw new Error(`${c.id} cli ${args[0]} --occupancy-frames: the counts differ`)
            if (fs.statSync(img).size !== 4 * c.n * c.width) throw new Error(`${c.id} cli: image size`)
        }
        // ... the rows need no bands; a threshold must be given, and only one
        fs.unlinkSync(outR)
        execFileSync(process.execPath, [...common, '--threshold-over-mean', String(c.overMean), '--occupancy-rows', outR], { stdio: 'pipe' })
        if (!sameWords(read(outR, Uint32Array), wants['.k'].rows)) throw new Error(`${c.id} cli --occupancy-rows without bands: the counts differ`)
        for (const args of [[], ['--threshold', '1', '--threshold-over-mean', '2'], ['--threshold', 'loud']]) {
            let failed = false
            try { execFileSync(process.execPath, [...common, ...args, '--occupancy-rows', outR], { stdio: 'pipe' }) } catch (e) { failed = e.status === 1 }
            if (!failed) throw new Error(`${c.id} cli: --occupancy-rows with [${args}] did not fail`)
        }

        // the refusals: a peak detector -4, bad bands and a bad threshold -1, in onerror / a throw and never in an array
        const refusals = [[{ detector: 'peak' }, { threshold, bands }, -4], [{}, { threshold, bands: [[0, c.n + 1]] }, -1],
            [{}, { threshold, bands: [[5, 4]] }, -1], [{}, { threshold, bands: [[0, 1.5]] }, -1], [{}, { threshold, bands: new Array(65).fill([0, 1]) }, -1],
            [{}, { threshold, bands: [0, 1, 2] }, -1], [{}, { threshold, bands: 7 }, -1], [{}, { bands }, -1], [{}, {}, -1],
            [{}, { threshold: threshold.subarray(1), bands }, -1], [{}, { threshold: new Float64Array(c.n + 1), bands }, -1],
            [{}, { threshold: Array.from(threshold), bands }, -1], [{}, { threshold: '1', bands }, -1]]
        for (const [extra, opt, status] of refusals) {
            let events = 0, seen
            worker.onerror = (e) => { events++; seen = e.status }
            let got = null, err = null
            try { got = await worker.renderOccupancy(Object.assign({}, message, extra), opt) } catch (e) { err = e }
            await new Promise(r => setImmediate(r))
            worker.onerror = null
            if (got !== null || !err || err.status !== status || events !== 1 || seen !== status)
                throw new Error(`${c.id}: ${JSON.stringify([extra, Object.keys(opt)])} was not refused with ${status} (${got}, ${err && err.status}, ${events}, ${seen})`)
            let thrown = null
            try { worker.renderOccupancySync(Object.assign({}, message, extra), opt) } catch (e) { thrown = e }
            if (!thrown || thrown.status !== status) throw new Error(`${c.id}: ${JSON.stringify([extra, Object.keys(opt)])} (sync) was not refused with ${status}`)
        }
        check(`${c.id} after the refusals`, await worker.renderOccupancy(message, { threshold, bands }), want, c, count)
    }
    worker.terminate()
    native.destroyContext(ctx)
    console.log(`occupancy ok: ${cases.length} cases`)
}

main(process.argv[2]).then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
