'use strict'
/**
 * What the N-API addon itself answers, asked directly (no HipWorker): its refusals - usage lines, handle, type and range errors - and the
 * shape of every reply kind.  EXPECT holds what the addon did before its reply kinds were folded into shared readers and writers, one line
 * per case; `node check_addon_shapes.js <cpu|gpu> --print` prints the lines of the code as it is.
 *
 *   cpu  no handle, no device: every render entry point without arguments and with ({}, {}), and the export table
 *   gpu  one context (and one group of [0]): per entry point the well-formed request - the reply's own properties in order, each with its
 *        type, length, FNV-1a digest, byteOffset and buffer.byteLength; under `stages` and `timings` the key names only (their values are
 *        times) and of `transportNote` the type only (the library's remark on the machine's transports) - its callback form, which must
 *        give the same line, the request with one field broken at a time, a group handle and a destroyed handle
 * The message is check_requests_cpu.js's: cu8, n = 64, width = 4, 512 bytes, a 2-entry colour map.  `render`, `renderNamed` and
 * `groupRender` read their numbers unchecked (a field that is no number keeps the value read before it); the table holds that too.
 */
const assert = require('assert')
const addon = require('../../spectroplot-js_amd/lib/spectroplot_hip.node')

// every name of the addon's Init table
const EXPORTS = ['deviceCount', 'parseFormat', 'window', 'sliceBounds', 'createContext', 'destroyContext', 'allocBuffer', 'poolStats', 'cmap',
    'cmapKeys', 'render', 'renderSync', 'renderNamed', 'renderNamedSync', 'renderBatch', 'renderBatchSync', 'renderTraces', 'renderTracesSync',
    'renderPower', 'renderPowerSync', 'renderMean', 'renderMeanSync', 'bandRows', 'renderBandPower', 'renderBandPowerSync', 'renderTrack',
    'renderTrackSync', 'renderOccupancy', 'renderOccupancySync', 'renderIndex', 'renderIndexSync', 'renderDensity', 'renderDensitySync',
    'namedResolve', 'peakSubframes', 'planCreations', 'createGroup', 'destroyGroup', 'groupRender', 'groupRenderSync']

// the render entry points: `name` takes a callback, `name`Sync does not
const KINDS = [
    { name: 'renderTraces', checked: true },
    { name: 'renderIndex', checked: true, picture: true },
    { name: 'renderDensity', checked: true, picture: true },
    { name: 'renderPower', checked: true, db: true },
    { name: 'renderMean', checked: true, db: true },
    { name: 'renderBandPower', checked: true, db: true, bands: true },
    { name: 'renderTrack', checked: true, db: true, bands: true },
    { name: 'renderOccupancy', checked: true, db: true, bands: true, threshold: true },
    { name: 'render', picture: true },
    { name: 'renderNamed', picture: true, named: true },
    { name: 'renderBatch', picture: true, batch: true },
    { name: 'groupRender', picture: true, group: true },
]

function fnv(bytes) {
    let h = 0x811c9dc5
    for (let i = 0; i < bytes.length; i++) h = Math.imul(h ^ bytes[i], 0x01000193) >>> 0
    return h.toString(16)
}
function show(v, key) {
    if (v instanceof ArrayBuffer) return `ArrayBuffer(${v.byteLength})#${fnv(new Uint8Array(v))}`
    if (ArrayBuffer.isView(v))
        return `${v.constructor.name}(${v.length})#${fnv(new Uint8Array(v.buffer, v.byteOffset, v.byteLength))} at ${v.byteOffset} of ${v.buffer.byteLength}`
    if (Array.isArray(v)) return '[' + v.map(e => show(e)).join(', ') + ']'
    if (typeof v === 'number' || typeof v === 'boolean') return `${typeof v} ${Object.is(v, -0) ? '-0' : String(v)}`
    if (typeof v === 'string') return key === 'transportNote' ? 'string' : `string ${JSON.stringify(v)}`
    if (v === null || typeof v !== 'object') return v === null ? 'null' : typeof v
    if (key === 'stages' || key === 'timings') return '{' + Object.getOwnPropertyNames(v).join(', ') + '}'
    let s = '{' + Object.getOwnPropertyNames(v).map(k => `${k}: ${show(v[k], k)}`).join(', ') + '}'
    if (v.trace_min && v.trace_max) s += ` trace_min.buffer === trace_max.buffer: ${v.trace_min.buffer === v.trace_max.buffer}`
    return s
}
const refusal = e => `${e.constructor.name} status ${show(e.status)}: ${e.message}`
function outcome(fn) {
    try { return show(fn()) } catch (e) { return refusal(e) }
}

const samples = new Uint8Array(1024)
for (let i = 0; i < samples.length; i++) samples[i] = (i * 37 + 11 + (i >> 8) * 5) & 255
const THRESHOLD = Float64Array.from({ length: 64 }, (_, y) => Math.pow(10, (y - 32) / 2))   // 1e-16 .. 3e15: below and above any |X|^2 here

function request(k) {
    const r = { format: addon.parseFormat('cu8').id, n: 64, width: 4, buffer: samples.buffer.slice(0, 512),
        windowc: Float64Array.from({ length: 64 }, (_, i) => 0.5 + i / 128), block_norm: 0.03125, gain: 6, range: 30, channelMode: false }
    if (k.picture) Object.assign(r, { lut: Uint8Array.from([0, 0, 0, 255, 255, 255]), waterfall: true, detector: 0 })
    if (k.named) {
        Object.assign(r, { format: 'cu8', window: 'hann', cmap: '0,0,0,255,255,255' })
        for (const f of ['windowc', 'block_norm', 'lut']) delete r[f]
    }
    if (k.db) r.db = true
    if (k.bands) r.bands = Int32Array.from([0, 8, 8, 64])
    if (k.threshold) r.threshold = Float64Array.from(THRESHOLD)
    if (k.batch) { delete r.buffer; delete r.width }
    return r
}
const items = () => [{ buffer: samples.buffer.slice(0, 512), width: 4 }, { buffer: samples.buffer.slice(512, 768), width: 2 }]
// the arguments of a kind's entry points behind the handle
const args = (k, req, its) => k.batch ? [req, its] : [req]

function breaks(k) {
    // a batch has `buffer` and `width` per item: broken in the first
    const set = (f, v) => (r, its) => { (k.batch && (f === 'buffer' || f === 'width') ? its[0] : r)[f] = v }
    const B = []
    for (const f of ['format', 'n', 'width', 'channelMode', 'block_norm', 'gain', 'range']) {
        B.push([`${f} a string`, set(f, '12')], [`${f} undefined`, set(f, undefined)])
        if (['format', 'n', 'width'].includes(f)) B.push([`${f} 1.5`, set(f, 1.5)])
    }
    B.push(['n 0', set('n', 0)], ['width -1', set('width', -1)])
    B.push(['windowc a plain Array', r => { r.windowc = Array.from(request({}).windowc) }],
        ['windowc a Float32Array', r => { r.windowc = Float32Array.from(request({}).windowc) }],
        ['windowc of 63 values', r => { r.windowc = request({}).windowc.slice(0, 63) }])
    B.push(['buffer missing', (r, its) => { delete (k.batch ? its[0] : r).buffer }], ['buffer a number', set('buffer', 7)])
    if (k.picture)
        B.push(['lut missing', r => { delete r.lut }], ['lut a Uint8ClampedArray', set('lut', Uint8ClampedArray.from([0, 0, 0, 255, 255, 255]))],
            ['lut of 2 bytes', set('lut', Uint8Array.from([0, 255]))], ['waterfall undefined', set('waterfall', undefined)],
            ['detector 2', set('detector', 2)], ["detector 'peak'", set('detector', 'peak')])
    if (k.db) B.push(['db undefined', set('db', undefined)])
    if (k.bands)
        B.push(['bands a plain Array', set('bands', [0, 8, 8, 64])], ['bands of odd length', set('bands', Int32Array.from([0, 8, 8]))],
            ['bands an Int32Array(0)', set('bands', new Int32Array(0))], ['bands of 65 pairs', set('bands', new Int32Array(130).map((_, i) => i & 1))],
            ['bands [0, 65]', set('bands', Int32Array.from([0, 65]))])
    if (k.threshold)
        B.push(['threshold missing', r => { delete r.threshold }], ['threshold a Float32Array', set('threshold', Float32Array.from(THRESHOLD))],
            ['threshold of 63 values', set('threshold', THRESHOLD.slice(0, 63))])
    if (k.batch)
        B.push(['items not an array', () => 'none'], ['an item that is a number', (r, its) => { its[1] = 7 }],
            ['an item with width -1', (r, its) => { its[1].width = -1 }], ['empty items', (r, its) => { its.length = 0 }])
    return B
}

const got = {}

function partA() {
    assert.strictEqual(EXPORTS.length, 40)
    for (const k of EXPORTS) assert.strictEqual(typeof addon[k], 'function', k)
    // the list is every name: what else the module object owns is `version`, a number
    assert.deepStrictEqual(Object.getOwnPropertyNames(addon).filter(k => typeof addon[k] === 'function').sort(), EXPORTS.slice().sort())
    got['exports: Object.keys'] = JSON.stringify(Object.keys(addon))
    got['exports: own properties that are no function'] =
        Object.getOwnPropertyNames(addon).filter(k => typeof addon[k] !== 'function').map(k => `${k}: ${typeof addon[k]}`).join(', ')
    for (const k of KINDS) {
        const cb = () => { throw new Error('a refused request called back') }
        got[`${k.name}Sync()`] = outcome(() => addon[k.name + 'Sync']())
        got[`${k.name}()`] = outcome(() => addon[k.name]())
        got[`${k.name}Sync({}, {})`] = outcome(() => addon[k.name + 'Sync']({}, {}))
        got[`${k.name}({}, {}, callback)`] = outcome(() => addon[k.name]({}, {}, cb))
        if (k.batch) {   // (its entry points take the items as a third argument)
            got[`${k.name}Sync({}, {}, [])`] = outcome(() => addon[k.name + 'Sync']({}, {}, []))
            got[`${k.name}({}, {}, [], callback)`] = outcome(() => addon[k.name]({}, {}, [], cb))
        }
    }
}

async function partB() {
    const ctx = addon.createContext(0), group = addon.createGroup([0])
    for (const k of KINDS) {
        const handle = k.group ? group : ctx
        const sync = (req, its) => outcome(() => addon[k.name + 'Sync'](handle, ...args(k, req, its)))
        const base = sync(request(k), items())
        got[`${k.name}Sync: well-formed`] = base
        if (k.threshold) {   // the threshold tells: the first row's is below every power, the last row's above
            const r = addon[k.name + 'Sync'](handle, request(k))
            assert.ok(r.rows[0] === 4 && r.rows[63] === 0, `occupancy rows ${r.rows[0]}, ${r.rows[63]}`)
        }
        const viaCallback = await new Promise(resolve => {
            try { addon[k.name](handle, ...args(k, request(k), items()), (err, r) => resolve(err ? refusal(err) : show(r))) } catch (e) { resolve(refusal(e)) }
        })
        assert.strictEqual(viaCallback, base, `${k.name}: the callback form's reply differs from the sync form's`)
        for (const [name, brk] of breaks(k)) {
            const req = request(k), its = items()
            const other = brk(req, its)   // (what takes the place of the items, if anything does)
            const line = sync(req, other === undefined ? its : other)
            got[`${k.name}Sync: ${name}`] = line === base ? 'as well-formed' : line
        }
    }
    for (const k of KINDS) if (k.checked || k.batch) got[`${k.name}Sync: a group handle`] = outcome(() => addon[k.name + 'Sync'](group, ...args(k, request(k), items())))
    addon.destroyContext(ctx)
    addon.destroyGroup(group)
    for (const k of KINDS) got[`${k.name}Sync: a destroyed handle`] = outcome(() => addon[k.name + 'Sync'](k.group ? group : ctx, ...args(k, request(k), items())))
}

const EXPECT = {
    cpu: {
        "exports: Object.keys": "[\"version\"]",
        "exports: own properties that are no function": "version: number",
        "renderTracesSync()": "TypeError status undefined: renderTracesSync(handle, request)",
        "renderTraces()": "TypeError status undefined: renderTraces(handle, request, callback)",
        "renderTracesSync({}, {})": "TypeError status undefined: context handle expected",
        "renderTraces({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderIndexSync()": "TypeError status undefined: renderIndexSync(handle, request)",
        "renderIndex()": "TypeError status undefined: renderIndex(handle, request, callback)",
        "renderIndexSync({}, {})": "TypeError status undefined: context handle expected",
        "renderIndex({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderDensitySync()": "TypeError status undefined: renderDensitySync(handle, request)",
        "renderDensity()": "TypeError status undefined: renderDensity(handle, request, callback)",
        "renderDensitySync({}, {})": "TypeError status undefined: context handle expected",
        "renderDensity({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderPowerSync()": "TypeError status undefined: renderPowerSync(handle, request)",
        "renderPower()": "TypeError status undefined: renderPower(handle, request, callback)",
        "renderPowerSync({}, {})": "TypeError status undefined: context handle expected",
        "renderPower({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderMeanSync()": "TypeError status undefined: renderMeanSync(handle, request)",
        "renderMean()": "TypeError status undefined: renderMean(handle, request, callback)",
        "renderMeanSync({}, {})": "TypeError status undefined: context handle expected",
        "renderMean({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderBandPowerSync()": "TypeError status undefined: renderBandPowerSync(handle, request)",
        "renderBandPower()": "TypeError status undefined: renderBandPower(handle, request, callback)",
        "renderBandPowerSync({}, {})": "TypeError status undefined: context handle expected",
        "renderBandPower({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderTrackSync()": "TypeError status undefined: renderTrackSync(handle, request)",
        "renderTrack()": "TypeError status undefined: renderTrack(handle, request, callback)",
        "renderTrackSync({}, {})": "TypeError status undefined: context handle expected",
        "renderTrack({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderOccupancySync()": "TypeError status undefined: renderOccupancySync(handle, request)",
        "renderOccupancy()": "TypeError status undefined: renderOccupancy(handle, request, callback)",
        "renderOccupancySync({}, {})": "TypeError status undefined: context handle expected",
        "renderOccupancy({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderSync()": "TypeError status undefined: context handle expected",
        "render()": "TypeError status undefined: context handle expected",
        "renderSync({}, {})": "TypeError status undefined: context handle expected",
        "render({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderNamedSync()": "TypeError status undefined: context handle expected",
        "renderNamed()": "TypeError status undefined: context handle expected",
        "renderNamedSync({}, {})": "TypeError status undefined: context handle expected",
        "renderNamed({}, {}, callback)": "TypeError status undefined: context handle expected",
        "renderBatchSync()": "TypeError status undefined: renderBatchSync(handle, request, items)",
        "renderBatch()": "TypeError status undefined: renderBatch(handle, request, items, callback)",
        "renderBatchSync({}, {})": "TypeError status undefined: renderBatchSync(handle, request, items)",
        "renderBatch({}, {}, callback)": "TypeError status undefined: renderBatch(handle, request, items, callback)",
        "renderBatchSync({}, {}, [])": "TypeError status undefined: context handle expected",
        "renderBatch({}, {}, [], callback)": "TypeError status undefined: context handle expected",
        "groupRenderSync()": "TypeError status undefined: context handle expected",
        "groupRender()": "TypeError status undefined: context handle expected",
        "groupRenderSync({}, {})": "TypeError status undefined: context handle expected",
        "groupRender({}, {}, callback)": "TypeError status undefined: context handle expected",
    },
    gpu: {
        "renderTracesSync: well-formed": "{trace_min: Float64Array(64)#9e3039b4 at 0 of 1024, trace_max: Float64Array(64)#80444b17 at 512 of 1024} trace_min.buffer === trace_max.buffer: true",
        "renderTracesSync: format a string": "TypeError status undefined: format must be a number",
        "renderTracesSync: format undefined": "TypeError status undefined: format must be a number",
        "renderTracesSync: format 1.5": "RangeError status undefined: format must be a 32-bit integer",
        "renderTracesSync: n a string": "TypeError status undefined: n must be a number",
        "renderTracesSync: n undefined": "TypeError status undefined: n must be a number",
        "renderTracesSync: n 1.5": "RangeError status undefined: n must be a 32-bit integer",
        "renderTracesSync: width a string": "TypeError status undefined: width must be a number",
        "renderTracesSync: width undefined": "TypeError status undefined: width must be a number",
        "renderTracesSync: width 1.5": "RangeError status undefined: width must be a 32-bit integer",
        "renderTracesSync: channelMode a string": "{trace_min: Float64Array(64)#fdd07843 at 0 of 1024, trace_max: Float64Array(64)#e743619c at 512 of 1024} trace_min.buffer === trace_max.buffer: true",
        "renderTracesSync: channelMode undefined": "as well-formed",
        "renderTracesSync: block_norm a string": "TypeError status undefined: block_norm must be a number",
        "renderTracesSync: block_norm undefined": "TypeError status undefined: block_norm must be a number",
        "renderTracesSync: gain a string": "TypeError status undefined: gain must be a number",
        "renderTracesSync: gain undefined": "TypeError status undefined: gain must be a number",
        "renderTracesSync: range a string": "TypeError status undefined: range must be a number",
        "renderTracesSync: range undefined": "TypeError status undefined: range must be a number",
        "renderTracesSync: n 0": "RangeError status undefined: n must be positive and width must not be negative",
        "renderTracesSync: width -1": "RangeError status undefined: n must be positive and width must not be negative",
        "renderTracesSync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderTracesSync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderTracesSync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderTracesSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderTracesSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderIndexSync: well-formed": "{index: Uint8Array(256)#9a7da265 at 0 of 256, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#7a62ba4a at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551}",
        "renderIndexSync: format a string": "TypeError status undefined: format must be a number",
        "renderIndexSync: format undefined": "TypeError status undefined: format must be a number",
        "renderIndexSync: format 1.5": "RangeError status undefined: format must be a 32-bit integer",
        "renderIndexSync: n a string": "TypeError status undefined: n must be a number",
        "renderIndexSync: n undefined": "TypeError status undefined: n must be a number",
        "renderIndexSync: n 1.5": "RangeError status undefined: n must be a 32-bit integer",
        "renderIndexSync: width a string": "TypeError status undefined: width must be a number",
        "renderIndexSync: width undefined": "TypeError status undefined: width must be a number",
        "renderIndexSync: width 1.5": "RangeError status undefined: width must be a 32-bit integer",
        "renderIndexSync: channelMode a string": "{index: Uint8Array(256)#aecd1d36 at 0 of 256, gauge_mins: ArrayBuffer(4)#4b95f515, gauge_maxs: ArrayBuffer(4)#998c1c65, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#803e9ffe at 0 of 16, cB_hist: Float64Array(1000)#273ff7f5 at 0 of 8000, dBfs_min: number -Infinity, dBfs_max: number -4.5389793905405185}",
        "renderIndexSync: channelMode undefined": "as well-formed",
        "renderIndexSync: block_norm a string": "TypeError status undefined: block_norm must be a number",
        "renderIndexSync: block_norm undefined": "TypeError status undefined: block_norm must be a number",
        "renderIndexSync: gain a string": "TypeError status undefined: gain must be a number",
        "renderIndexSync: gain undefined": "TypeError status undefined: gain must be a number",
        "renderIndexSync: range a string": "TypeError status undefined: range must be a number",
        "renderIndexSync: range undefined": "TypeError status undefined: range must be a number",
        "renderIndexSync: n 0": "RangeError status undefined: n must be positive and width must not be negative",
        "renderIndexSync: width -1": "RangeError status undefined: n must be positive and width must not be negative",
        "renderIndexSync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderIndexSync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderIndexSync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderIndexSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderIndexSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderIndexSync: lut missing": "TypeError status undefined: lut must be a Uint8Array of r, g, b triples",
        "renderIndexSync: lut a Uint8ClampedArray": "as well-formed",
        "renderIndexSync: lut of 2 bytes": "TypeError status undefined: lut must be a Uint8Array of r, g, b triples",
        "renderIndexSync: waterfall undefined": "{index: Uint8Array(256)#2b714671 at 0 of 256, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#7a62ba4a at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551}",
        "renderIndexSync: detector 2": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderIndexSync: detector 'peak'": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderDensitySync: well-formed": "{density: Uint32Array(128)#8c73825 at 0 of 512, n: number 64, lutLen: number 2, width: number 4}",
        "renderDensitySync: format a string": "TypeError status undefined: format must be a number",
        "renderDensitySync: format undefined": "TypeError status undefined: format must be a number",
        "renderDensitySync: format 1.5": "RangeError status undefined: format must be a 32-bit integer",
        "renderDensitySync: n a string": "TypeError status undefined: n must be a number",
        "renderDensitySync: n undefined": "TypeError status undefined: n must be a number",
        "renderDensitySync: n 1.5": "RangeError status undefined: n must be a 32-bit integer",
        "renderDensitySync: width a string": "TypeError status undefined: width must be a number",
        "renderDensitySync: width undefined": "TypeError status undefined: width must be a number",
        "renderDensitySync: width 1.5": "RangeError status undefined: width must be a 32-bit integer",
        "renderDensitySync: channelMode a string": "{density: Uint32Array(128)#87f6e473 at 0 of 512, n: number 64, lutLen: number 2, width: number 4}",
        "renderDensitySync: channelMode undefined": "as well-formed",
        "renderDensitySync: block_norm a string": "TypeError status undefined: block_norm must be a number",
        "renderDensitySync: block_norm undefined": "TypeError status undefined: block_norm must be a number",
        "renderDensitySync: gain a string": "TypeError status undefined: gain must be a number",
        "renderDensitySync: gain undefined": "TypeError status undefined: gain must be a number",
        "renderDensitySync: range a string": "TypeError status undefined: range must be a number",
        "renderDensitySync: range undefined": "TypeError status undefined: range must be a number",
        "renderDensitySync: n 0": "RangeError status undefined: n must be positive and width must not be negative",
        "renderDensitySync: width -1": "RangeError status undefined: n must be positive and width must not be negative",
        "renderDensitySync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderDensitySync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderDensitySync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderDensitySync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderDensitySync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderDensitySync: lut missing": "TypeError status undefined: lut must be a Uint8Array of r, g, b triples",
        "renderDensitySync: lut a Uint8ClampedArray": "as well-formed",
        "renderDensitySync: lut of 2 bytes": "TypeError status undefined: lut must be a Uint8Array of r, g, b triples",
        "renderDensitySync: waterfall undefined": "as well-formed",
        "renderDensitySync: detector 2": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderDensitySync: detector 'peak'": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderPowerSync: well-formed": "{power: Float64Array(256)#fe62efa4 at 0 of 2048, width: number 4, n: number 64}",
        "renderPowerSync: format a string": "TypeError status undefined: format must be a number",
        "renderPowerSync: format undefined": "TypeError status undefined: format must be a number",
        "renderPowerSync: format 1.5": "RangeError status undefined: format must be a 32-bit integer",
        "renderPowerSync: n a string": "TypeError status undefined: n must be a number",
        "renderPowerSync: n undefined": "TypeError status undefined: n must be a number",
        "renderPowerSync: n 1.5": "RangeError status undefined: n must be a 32-bit integer",
        "renderPowerSync: width a string": "TypeError status undefined: width must be a number",
        "renderPowerSync: width undefined": "TypeError status undefined: width must be a number",
        "renderPowerSync: width 1.5": "RangeError status undefined: width must be a 32-bit integer",
        "renderPowerSync: channelMode a string": "{power: Float64Array(256)#e3400ebb at 0 of 2048, width: number 4, n: number 64}",
        "renderPowerSync: channelMode undefined": "as well-formed",
        "renderPowerSync: block_norm a string": "TypeError status undefined: block_norm must be a number",
        "renderPowerSync: block_norm undefined": "TypeError status undefined: block_norm must be a number",
        "renderPowerSync: gain a string": "TypeError status undefined: gain must be a number",
        "renderPowerSync: gain undefined": "TypeError status undefined: gain must be a number",
        "renderPowerSync: range a string": "TypeError status undefined: range must be a number",
        "renderPowerSync: range undefined": "TypeError status undefined: range must be a number",
        "renderPowerSync: n 0": "RangeError status undefined: n must be positive and width must not be negative",
        "renderPowerSync: width -1": "RangeError status undefined: n must be positive and width must not be negative",
        "renderPowerSync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderPowerSync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderPowerSync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderPowerSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderPowerSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderPowerSync: db undefined": "{power: Float64Array(256)#999a38ee at 0 of 2048, width: number 4, n: number 64}",
        "renderMeanSync: well-formed": "{mean: Float64Array(64)#e89619b9 at 0 of 512, width: number 4, n: number 64}",
        "renderMeanSync: format a string": "TypeError status undefined: format must be a number",
        "renderMeanSync: format undefined": "TypeError status undefined: format must be a number",
        "renderMeanSync: format 1.5": "RangeError status undefined: format must be a 32-bit integer",
        "renderMeanSync: n a string": "TypeError status undefined: n must be a number",
        "renderMeanSync: n undefined": "TypeError status undefined: n must be a number",
        "renderMeanSync: n 1.5": "RangeError status undefined: n must be a 32-bit integer",
        "renderMeanSync: width a string": "TypeError status undefined: width must be a number",
        "renderMeanSync: width undefined": "TypeError status undefined: width must be a number",
        "renderMeanSync: width 1.5": "RangeError status undefined: width must be a 32-bit integer",
        "renderMeanSync: channelMode a string": "{mean: Float64Array(64)#35cb9201 at 0 of 512, width: number 4, n: number 64}",
        "renderMeanSync: channelMode undefined": "as well-formed",
        "renderMeanSync: block_norm a string": "TypeError status undefined: block_norm must be a number",
        "renderMeanSync: block_norm undefined": "TypeError status undefined: block_norm must be a number",
        "renderMeanSync: gain a string": "TypeError status undefined: gain must be a number",
        "renderMeanSync: gain undefined": "TypeError status undefined: gain must be a number",
        "renderMeanSync: range a string": "TypeError status undefined: range must be a number",
        "renderMeanSync: range undefined": "TypeError status undefined: range must be a number",
        "renderMeanSync: n 0": "RangeError status undefined: n must be positive and width must not be negative",
        "renderMeanSync: width -1": "RangeError status undefined: n must be positive and width must not be negative",
        "renderMeanSync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderMeanSync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderMeanSync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderMeanSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderMeanSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderMeanSync: db undefined": "{mean: Float64Array(64)#84fd547a at 0 of 512, width: number 4, n: number 64}",
        "renderBandPowerSync: well-formed": "{bands: Float64Array(8)#141dcfe at 0 of 64, count: number 2, width: number 4, n: number 64}",
        "renderBandPowerSync: format a string": "TypeError status undefined: format must be a number",
        "renderBandPowerSync: format undefined": "TypeError status undefined: format must be a number",
        "renderBandPowerSync: format 1.5": "RangeError status undefined: format must be a 32-bit integer",
        "renderBandPowerSync: n a string": "TypeError status undefined: n must be a number",
        "renderBandPowerSync: n undefined": "TypeError status undefined: n must be a number",
        "renderBandPowerSync: n 1.5": "RangeError status undefined: n must be a 32-bit integer",
        "renderBandPowerSync: width a string": "TypeError status undefined: width must be a number",
        "renderBandPowerSync: width undefined": "TypeError status undefined: width must be a number",
        "renderBandPowerSync: width 1.5": "RangeError status undefined: width must be a 32-bit integer",
        "renderBandPowerSync: channelMode a string": "{bands: Float64Array(8)#56299496 at 0 of 64, count: number 2, width: number 4, n: number 64}",
        "renderBandPowerSync: channelMode undefined": "as well-formed",
        "renderBandPowerSync: block_norm a string": "TypeError status undefined: block_norm must be a number",
        "renderBandPowerSync: block_norm undefined": "TypeError status undefined: block_norm must be a number",
        "renderBandPowerSync: gain a string": "TypeError status undefined: gain must be a number",
        "renderBandPowerSync: gain undefined": "TypeError status undefined: gain must be a number",
        "renderBandPowerSync: range a string": "TypeError status undefined: range must be a number",
        "renderBandPowerSync: range undefined": "TypeError status undefined: range must be a number",
        "renderBandPowerSync: n 0": "RangeError status undefined: n must be positive and width must not be negative",
        "renderBandPowerSync: width -1": "RangeError status undefined: n must be positive and width must not be negative",
        "renderBandPowerSync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderBandPowerSync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderBandPowerSync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderBandPowerSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderBandPowerSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderBandPowerSync: db undefined": "{bands: Float64Array(8)#77484f2f at 0 of 64, count: number 2, width: number 4, n: number 64}",
        "renderBandPowerSync: bands a plain Array": "TypeError status undefined: bands must be an Int32Array of y0, y1 pairs",
        "renderBandPowerSync: bands of odd length": "TypeError status undefined: bands must be an Int32Array of y0, y1 pairs",
        "renderBandPowerSync: bands an Int32Array(0)": "{bands: Float64Array(0)#811c9dc5 at 0 of 0, count: number 0, width: number 4, n: number 64}",
        "renderBandPowerSync: bands of 65 pairs": "Error status number -1: count must be 0 .. SP_MAX_BANDS",
        "renderBandPowerSync: bands [0, 65]": "Error status number -1: a band must satisfy 0 <= y0 <= y1 <= n",
        "renderTrackSync: well-formed": "{rows: Int32Array(8)#91a8f114 at 0 of 32, peaks: Float64Array(8)#acc3f3bb at 0 of 64, count: number 2, width: number 4, n: number 64}",
        "renderTrackSync: format a string": "TypeError status undefined: format must be a number",
        "renderTrackSync: format undefined": "TypeError status undefined: format must be a number",
        "renderTrackSync: format 1.5": "RangeError status undefined: format must be a 32-bit integer",
        "renderTrackSync: n a string": "TypeError status undefined: n must be a number",
        "renderTrackSync: n undefined": "TypeError status undefined: n must be a number",
        "renderTrackSync: n 1.5": "RangeError status undefined: n must be a 32-bit integer",
        "renderTrackSync: width a string": "TypeError status undefined: width must be a number",
        "renderTrackSync: width undefined": "TypeError status undefined: width must be a number",
        "renderTrackSync: width 1.5": "RangeError status undefined: width must be a 32-bit integer",
        "renderTrackSync: channelMode a string": "{rows: Int32Array(8)#b5cb2e65 at 0 of 32, peaks: Float64Array(8)#2584f37a at 0 of 64, count: number 2, width: number 4, n: number 64}",
        "renderTrackSync: channelMode undefined": "as well-formed",
        "renderTrackSync: block_norm a string": "TypeError status undefined: block_norm must be a number",
        "renderTrackSync: block_norm undefined": "TypeError status undefined: block_norm must be a number",
        "renderTrackSync: gain a string": "TypeError status undefined: gain must be a number",
        "renderTrackSync: gain undefined": "TypeError status undefined: gain must be a number",
        "renderTrackSync: range a string": "TypeError status undefined: range must be a number",
        "renderTrackSync: range undefined": "TypeError status undefined: range must be a number",
        "renderTrackSync: n 0": "RangeError status undefined: n must be positive and width must not be negative",
        "renderTrackSync: width -1": "RangeError status undefined: n must be positive and width must not be negative",
        "renderTrackSync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderTrackSync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderTrackSync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderTrackSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderTrackSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderTrackSync: db undefined": "{rows: Int32Array(8)#91a8f114 at 0 of 32, peaks: Float64Array(8)#ba8d57e1 at 0 of 64, count: number 2, width: number 4, n: number 64}",
        "renderTrackSync: bands a plain Array": "TypeError status undefined: bands must be an Int32Array of y0, y1 pairs",
        "renderTrackSync: bands of odd length": "TypeError status undefined: bands must be an Int32Array of y0, y1 pairs",
        "renderTrackSync: bands an Int32Array(0)": "{rows: Int32Array(0)#811c9dc5 at 0 of 0, peaks: Float64Array(0)#811c9dc5 at 0 of 0, count: number 0, width: number 4, n: number 64}",
        "renderTrackSync: bands of 65 pairs": "Error status number -1: count must be 0 .. SP_MAX_BANDS",
        "renderTrackSync: bands [0, 65]": "Error status number -1: a band must satisfy 0 <= y0 <= y1 <= n",
        "renderOccupancySync: well-formed": "{rows: Uint32Array(64)#2f713a87 at 0 of 256, frames: Uint32Array(8)#e88db2c5 at 0 of 32, count: number 2, width: number 4, n: number 64}",
        "renderOccupancySync: format a string": "TypeError status undefined: format must be a number",
        "renderOccupancySync: format undefined": "TypeError status undefined: format must be a number",
        "renderOccupancySync: format 1.5": "RangeError status undefined: format must be a 32-bit integer",
        "renderOccupancySync: n a string": "TypeError status undefined: n must be a number",
        "renderOccupancySync: n undefined": "TypeError status undefined: n must be a number",
        "renderOccupancySync: n 1.5": "RangeError status undefined: n must be a 32-bit integer",
        "renderOccupancySync: width a string": "TypeError status undefined: width must be a number",
        "renderOccupancySync: width undefined": "TypeError status undefined: width must be a number",
        "renderOccupancySync: width 1.5": "RangeError status undefined: width must be a 32-bit integer",
        "renderOccupancySync: channelMode a string": "{rows: Uint32Array(64)#ea5f33c0 at 0 of 256, frames: Uint32Array(8)#2d3e3cd4 at 0 of 32, count: number 2, width: number 4, n: number 64}",
        "renderOccupancySync: channelMode undefined": "as well-formed",
        "renderOccupancySync: block_norm a string": "TypeError status undefined: block_norm must be a number",
        "renderOccupancySync: block_norm undefined": "TypeError status undefined: block_norm must be a number",
        "renderOccupancySync: gain a string": "TypeError status undefined: gain must be a number",
        "renderOccupancySync: gain undefined": "TypeError status undefined: gain must be a number",
        "renderOccupancySync: range a string": "TypeError status undefined: range must be a number",
        "renderOccupancySync: range undefined": "TypeError status undefined: range must be a number",
        "renderOccupancySync: n 0": "RangeError status undefined: n must be positive and width must not be negative",
        "renderOccupancySync: width -1": "RangeError status undefined: n must be positive and width must not be negative",
        "renderOccupancySync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderOccupancySync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderOccupancySync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderOccupancySync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderOccupancySync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderOccupancySync: db undefined": "as well-formed",
        "renderOccupancySync: bands a plain Array": "TypeError status undefined: bands must be an Int32Array of y0, y1 pairs",
        "renderOccupancySync: bands of odd length": "TypeError status undefined: bands must be an Int32Array of y0, y1 pairs",
        "renderOccupancySync: bands an Int32Array(0)": "{rows: Uint32Array(64)#2f713a87 at 0 of 256, frames: Uint32Array(0)#811c9dc5 at 0 of 0, count: number 0, width: number 4, n: number 64}",
        "renderOccupancySync: bands of 65 pairs": "Error status number -1: count must be 0 .. SP_MAX_BANDS",
        "renderOccupancySync: bands [0, 65]": "Error status number -1: a band must satisfy 0 <= y0 <= y1 <= n",
        "renderOccupancySync: threshold missing": "TypeError status undefined: threshold must be a Float64Array of n powers",
        "renderOccupancySync: threshold a Float32Array": "TypeError status undefined: threshold must be a Float64Array of n powers",
        "renderOccupancySync: threshold of 63 values": "Error status number -1: threshold must hold n values, one per image row",
        "renderSync: well-formed": "{rgba: ArrayBuffer(1024)#5dafc105, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#7a62ba4a at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551}",
        "renderSync: format a string": "{rgba: ArrayBuffer(1024)#46f61e9d, gauge_mins: ArrayBuffer(4)#8590c5a5, gauge_maxs: ArrayBuffer(4)#c26e86a6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#b8396a68 at 0 of 16, cB_hist: Float64Array(1000)#d3fc60bc at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -24.732104172541845, dBfs_max: number -2.5318733492631065}",
        "renderSync: format undefined": "{rgba: ArrayBuffer(1024)#46f61e9d, gauge_mins: ArrayBuffer(4)#8590c5a5, gauge_maxs: ArrayBuffer(4)#c26e86a6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#b8396a68 at 0 of 16, cB_hist: Float64Array(1000)#d3fc60bc at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -24.732104172541845, dBfs_max: number -2.5318733492631065}",
        "renderSync: format 1.5": "{rgba: ArrayBuffer(1024)#90e0ad7c, gauge_mins: ArrayBuffer(4)#e9fb8925, gauge_maxs: ArrayBuffer(4)#c0d9b535, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#9a725708 at 0 of 16, cB_hist: Float64Array(1000)#c63a12d4 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -21.964914290808423, dBfs_max: number -2.792747642499007}",
        "renderSync: n a string": "{rgba: ArrayBuffer(32)#4bff0505, gauge_mins: ArrayBuffer(4)#79188162, gauge_maxs: ArrayBuffer(4)#4f06fc92, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#cc9126e5 at 0 of 16, cB_hist: Float64Array(1000)#ef2350e5 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -18.94146505909766, dBfs_max: number -16.133799447167874}",
        "renderSync: n undefined": "{rgba: ArrayBuffer(32)#4bff0505, gauge_mins: ArrayBuffer(4)#79188162, gauge_maxs: ArrayBuffer(4)#4f06fc92, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#cc9126e5 at 0 of 16, cB_hist: Float64Array(1000)#ef2350e5 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -18.94146505909766, dBfs_max: number -16.133799447167874}",
        "renderSync: n 1.5": "Error status number -4: n = 1 is not supported (the reference writes no pixels for it)",
        "renderSync: width a string": "{rgba: ArrayBuffer(16384)#9147722c, gauge_mins: ArrayBuffer(64)#8e3eb7ad, gauge_maxs: ArrayBuffer(64)#13e5640c, gauge_amps: ArrayBuffer(64)#ea390d39, c_hist: Float64Array(2)#8bcb3824 at 0 of 16, cB_hist: Float64Array(1000)#28b5b74 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -29.09366424828376, dBfs_max: number -1.6994747766569187}",
        "renderSync: width undefined": "{rgba: ArrayBuffer(16384)#9147722c, gauge_mins: ArrayBuffer(64)#8e3eb7ad, gauge_maxs: ArrayBuffer(64)#13e5640c, gauge_amps: ArrayBuffer(64)#ea390d39, c_hist: Float64Array(2)#8bcb3824 at 0 of 16, cB_hist: Float64Array(1000)#28b5b74 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -29.09366424828376, dBfs_max: number -1.6994747766569187}",
        "renderSync: width 1.5": "{rgba: ArrayBuffer(256)#d9506094, gauge_mins: ArrayBuffer(1)#ca0c003e, gauge_maxs: ArrayBuffer(1)#680b65f8, gauge_amps: ArrayBuffer(1)#7a0b824e, c_hist: Float64Array(2)#48264968 at 0 of 16, cB_hist: Float64Array(1000)#8383dcc5 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -20.80571986754217, dBfs_max: number -2.285438743784166}",
        "renderSync: channelMode a string": "{rgba: ArrayBuffer(1024)#20c583f4, gauge_mins: ArrayBuffer(4)#4b95f515, gauge_maxs: ArrayBuffer(4)#998c1c65, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#803e9ffe at 0 of 16, cB_hist: Float64Array(1000)#273ff7f5 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -Infinity, dBfs_max: number -4.5389793905405185}",
        "renderSync: channelMode undefined": "as well-formed",
        "renderSync: block_norm a string": "{rgba: ArrayBuffer(1024)#c3705c5, gauge_mins: ArrayBuffer(4)#4b95f515, gauge_maxs: ArrayBuffer(4)#4b95f515, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#6604e095 at 0 of 16, cB_hist: Float64Array(1000)#772d4a55 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -Infinity, dBfs_max: number -200}",
        "renderSync: block_norm undefined": "{rgba: ArrayBuffer(1024)#c3705c5, gauge_mins: ArrayBuffer(4)#4b95f515, gauge_maxs: ArrayBuffer(4)#4b95f515, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#6604e095 at 0 of 16, cB_hist: Float64Array(1000)#772d4a55 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -Infinity, dBfs_max: number -200}",
        "renderSync: gain a string": "{rgba: ArrayBuffer(1024)#d6fdbb64, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#ea0a44d9, c_hist: Float64Array(2)#ca095d46 at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551}",
        "renderSync: gain undefined": "{rgba: ArrayBuffer(1024)#d6fdbb64, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#ea0a44d9, c_hist: Float64Array(2)#ca095d46 at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551}",
        "renderSync: range a string": "Error status number -4: range must be finite and > 0",
        "renderSync: range undefined": "Error status number -4: range must be finite and > 0",
        "renderSync: n 0": "Error status number -2: Length is not a power of 2",
        "renderSync: width -1": "Error status number -1: width < 0",
        "renderSync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderSync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderSync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderSync: lut missing": "TypeError status undefined: lut must be a Uint8Array",
        "renderSync: lut a Uint8ClampedArray": "as well-formed",
        "renderSync: lut of 2 bytes": "Error status number -4: lut_len must be 1..SP_MAX_LUT",
        "renderSync: waterfall undefined": "{rgba: ArrayBuffer(1024)#23263895, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#7a62ba4a at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551}",
        "renderSync: detector 2": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderSync: detector 'peak'": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderNamedSync: well-formed": "{rgba: ArrayBuffer(1024)#86f3bb4, gauge_mins: ArrayBuffer(4)#700159e, gauge_maxs: ArrayBuffer(4)#6d828241, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(256)#8d8985e2 at 0 of 2048, cB_hist: Float64Array(1000)#8e428fc1 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -24.581853117678847, dBfs_max: number -2.413739550875876}",
        "renderNamedSync: format a string": "as well-formed",
        "renderNamedSync: format undefined": "as well-formed",
        "renderNamedSync: format 1.5": "as well-formed",
        "renderNamedSync: n a string": "Error status number -2: Length is not a power of 2",
        "renderNamedSync: n undefined": "Error status number -2: Length is not a power of 2",
        "renderNamedSync: n 1.5": "Error status number -4: n = 1 is not supported (the reference writes no pixels for it)",
        "renderNamedSync: width a string": "{rgba: ArrayBuffer(16384)#8188188f, gauge_mins: ArrayBuffer(64)#ea3128f2, gauge_maxs: ArrayBuffer(64)#59bb2dff, gauge_amps: ArrayBuffer(64)#ea390d39, c_hist: Float64Array(256)#9037b2e at 0 of 2048, cB_hist: Float64Array(1000)#ec609025 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -33.090525427149565, dBfs_max: number -2.390908030614904}",
        "renderNamedSync: width undefined": "{rgba: ArrayBuffer(16384)#8188188f, gauge_mins: ArrayBuffer(64)#ea3128f2, gauge_maxs: ArrayBuffer(64)#59bb2dff, gauge_amps: ArrayBuffer(64)#ea390d39, c_hist: Float64Array(256)#9037b2e at 0 of 2048, cB_hist: Float64Array(1000)#ec609025 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -33.090525427149565, dBfs_max: number -2.390908030614904}",
        "renderNamedSync: width 1.5": "{rgba: ArrayBuffer(256)#a1633187, gauge_mins: ArrayBuffer(1)#2a0c975e, gauge_maxs: ArrayBuffer(1)#6f0b70fd, gauge_amps: ArrayBuffer(1)#7a0b824e, c_hist: Float64Array(256)#8ef65a45 at 0 of 2048, cB_hist: Float64Array(1000)#61bd4460 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -24.581853117678847, dBfs_max: number -2.664221824785015}",
        "renderNamedSync: channelMode a string": "{rgba: ArrayBuffer(1024)#14fa73f2, gauge_mins: ArrayBuffer(4)#4b95f515, gauge_maxs: ArrayBuffer(4)#2a125962, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(256)#7f29ebe7 at 0 of 2048, cB_hist: Float64Array(1000)#c8b5187e at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -Infinity, dBfs_max: number -5.150736467413511}",
        "renderNamedSync: channelMode undefined": "as well-formed",
        "renderNamedSync: block_norm a string": "as well-formed",
        "renderNamedSync: block_norm undefined": "as well-formed",
        "renderNamedSync: gain a string": "{rgba: ArrayBuffer(1024)#a1db7977, gauge_mins: ArrayBuffer(4)#700159e, gauge_maxs: ArrayBuffer(4)#6d828241, gauge_amps: ArrayBuffer(4)#ea0a44d9, c_hist: Float64Array(256)#3e5119cd at 0 of 2048, cB_hist: Float64Array(1000)#8e428fc1 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -24.581853117678847, dBfs_max: number -2.413739550875876}",
        "renderNamedSync: gain undefined": "{rgba: ArrayBuffer(1024)#a1db7977, gauge_mins: ArrayBuffer(4)#700159e, gauge_maxs: ArrayBuffer(4)#6d828241, gauge_amps: ArrayBuffer(4)#ea0a44d9, c_hist: Float64Array(256)#3e5119cd at 0 of 2048, cB_hist: Float64Array(1000)#8e428fc1 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -24.581853117678847, dBfs_max: number -2.413739550875876}",
        "renderNamedSync: range a string": "Error status number -4: range must be finite and > 0",
        "renderNamedSync: range undefined": "Error status number -4: range must be finite and > 0",
        "renderNamedSync: n 0": "Error status number -2: Length is not a power of 2",
        "renderNamedSync: width -1": "Error status number -1: width < 0",
        "renderNamedSync: windowc a plain Array": "as well-formed",
        "renderNamedSync: windowc a Float32Array": "as well-formed",
        "renderNamedSync: windowc of 63 values": "as well-formed",
        "renderNamedSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderNamedSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderNamedSync: lut missing": "as well-formed",
        "renderNamedSync: lut a Uint8ClampedArray": "as well-formed",
        "renderNamedSync: lut of 2 bytes": "as well-formed",
        "renderNamedSync: waterfall undefined": "{rgba: ArrayBuffer(1024)#f391092c, gauge_mins: ArrayBuffer(4)#700159e, gauge_maxs: ArrayBuffer(4)#6d828241, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(256)#8d8985e2 at 0 of 2048, cB_hist: Float64Array(1000)#8e428fc1 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -24.581853117678847, dBfs_max: number -2.413739550875876}",
        "renderNamedSync: detector 2": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderNamedSync: detector 'peak'": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderBatchSync: well-formed": "[{rgba: ArrayBuffer(1024)#5dafc105, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#7a62ba4a at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551}, {rgba: ArrayBuffer(512)#31e21845, gauge_mins: ArrayBuffer(2)#2fbe2a22, gauge_maxs: ArrayBuffer(2)#def86ed4, gauge_amps: ArrayBuffer(2)#d11ebca3, c_hist: Float64Array(2)#91beb6d3 at 0 of 16, cB_hist: Float64Array(1000)#24137995 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -25.470237950966087, dBfs_max: number -2.161039304882287}]",
        "renderBatchSync: format a string": "TypeError status undefined: format must be a number",
        "renderBatchSync: format undefined": "TypeError status undefined: format must be a number",
        "renderBatchSync: format 1.5": "RangeError status undefined: format must be a 32-bit integer",
        "renderBatchSync: n a string": "TypeError status undefined: n must be a number",
        "renderBatchSync: n undefined": "TypeError status undefined: n must be a number",
        "renderBatchSync: n 1.5": "RangeError status undefined: n must be a 32-bit integer",
        "renderBatchSync: width a string": "TypeError status undefined: width must be a number",
        "renderBatchSync: width undefined": "TypeError status undefined: width must be a number",
        "renderBatchSync: width 1.5": "RangeError status undefined: width must be a 32-bit integer",
        "renderBatchSync: channelMode a string": "[{rgba: ArrayBuffer(1024)#20c583f4, gauge_mins: ArrayBuffer(4)#4b95f515, gauge_maxs: ArrayBuffer(4)#998c1c65, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#803e9ffe at 0 of 16, cB_hist: Float64Array(1000)#273ff7f5 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -Infinity, dBfs_max: number -4.5389793905405185}, {rgba: ArrayBuffer(512)#b0ef4f64, gauge_mins: ArrayBuffer(2)#117697cd, gauge_maxs: ArrayBuffer(2)#b9da1f81, gauge_amps: ArrayBuffer(2)#d11ebca3, c_hist: Float64Array(2)#eb3e37be at 0 of 16, cB_hist: Float64Array(1000)#f0f94d85 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -Infinity, dBfs_max: number -4.547365952985489}]",
        "renderBatchSync: channelMode undefined": "as well-formed",
        "renderBatchSync: block_norm a string": "TypeError status undefined: block_norm must be a number",
        "renderBatchSync: block_norm undefined": "TypeError status undefined: block_norm must be a number",
        "renderBatchSync: gain a string": "TypeError status undefined: gain must be a number",
        "renderBatchSync: gain undefined": "TypeError status undefined: gain must be a number",
        "renderBatchSync: range a string": "TypeError status undefined: range must be a number",
        "renderBatchSync: range undefined": "TypeError status undefined: range must be a number",
        "renderBatchSync: n 0": "Error status number -2: Length is not a power of 2",
        "renderBatchSync: width -1": "RangeError status undefined: width must not be negative",
        "renderBatchSync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderBatchSync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "renderBatchSync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "renderBatchSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderBatchSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "renderBatchSync: lut missing": "TypeError status undefined: lut must be a Uint8Array",
        "renderBatchSync: lut a Uint8ClampedArray": "as well-formed",
        "renderBatchSync: lut of 2 bytes": "Error status number -4: lut_len must be 1..SP_MAX_LUT",
        "renderBatchSync: waterfall undefined": "[{rgba: ArrayBuffer(1024)#23263895, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#7a62ba4a at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551}, {rgba: ArrayBuffer(512)#b99c2f45, gauge_mins: ArrayBuffer(2)#2fbe2a22, gauge_maxs: ArrayBuffer(2)#def86ed4, gauge_amps: ArrayBuffer(2)#d11ebca3, c_hist: Float64Array(2)#91beb6d3 at 0 of 16, cB_hist: Float64Array(1000)#24137995 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -25.470237950966087, dBfs_max: number -2.161039304882287}]",
        "renderBatchSync: detector 2": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderBatchSync: detector 'peak'": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderBatchSync: items not an array": "TypeError status undefined: items must be an array of {buffer, width}",
        "renderBatchSync: an item that is a number": "TypeError status undefined: items must be an array of {buffer, width}",
        "renderBatchSync: an item with width -1": "RangeError status undefined: width must not be negative",
        "renderBatchSync: empty items": "[]",
        "groupRenderSync: well-formed": "{rgba: ArrayBuffer(1024)#5dafc105, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#7a62ba4a at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: format a string": "{rgba: ArrayBuffer(1024)#46f61e9d, gauge_mins: ArrayBuffer(4)#8590c5a5, gauge_maxs: ArrayBuffer(4)#c26e86a6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#b8396a68 at 0 of 16, cB_hist: Float64Array(1000)#d3fc60bc at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -24.732104172541845, dBfs_max: number -2.5318733492631065, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: format undefined": "{rgba: ArrayBuffer(1024)#46f61e9d, gauge_mins: ArrayBuffer(4)#8590c5a5, gauge_maxs: ArrayBuffer(4)#c26e86a6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#b8396a68 at 0 of 16, cB_hist: Float64Array(1000)#d3fc60bc at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -24.732104172541845, dBfs_max: number -2.5318733492631065, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: format 1.5": "{rgba: ArrayBuffer(1024)#90e0ad7c, gauge_mins: ArrayBuffer(4)#e9fb8925, gauge_maxs: ArrayBuffer(4)#c0d9b535, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#9a725708 at 0 of 16, cB_hist: Float64Array(1000)#c63a12d4 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -21.964914290808423, dBfs_max: number -2.792747642499007, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: n a string": "{rgba: ArrayBuffer(32)#4bff0505, gauge_mins: ArrayBuffer(4)#79188162, gauge_maxs: ArrayBuffer(4)#4f06fc92, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#cc9126e5 at 0 of 16, cB_hist: Float64Array(1000)#ef2350e5 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -18.94146505909766, dBfs_max: number -16.133799447167874, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: n undefined": "{rgba: ArrayBuffer(32)#4bff0505, gauge_mins: ArrayBuffer(4)#79188162, gauge_maxs: ArrayBuffer(4)#4f06fc92, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#cc9126e5 at 0 of 16, cB_hist: Float64Array(1000)#ef2350e5 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -18.94146505909766, dBfs_max: number -16.133799447167874, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: n 1.5": "Error status number -4: n = 1 is not supported (the reference writes no pixels for it)",
        "groupRenderSync: width a string": "{rgba: ArrayBuffer(16384)#9147722c, gauge_mins: ArrayBuffer(64)#8e3eb7ad, gauge_maxs: ArrayBuffer(64)#13e5640c, gauge_amps: ArrayBuffer(64)#ea390d39, c_hist: Float64Array(2)#8bcb3824 at 0 of 16, cB_hist: Float64Array(1000)#28b5b74 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -29.09366424828376, dBfs_max: number -1.6994747766569187, members: number 1, sliceWidth: number 64, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: width undefined": "{rgba: ArrayBuffer(16384)#9147722c, gauge_mins: ArrayBuffer(64)#8e3eb7ad, gauge_maxs: ArrayBuffer(64)#13e5640c, gauge_amps: ArrayBuffer(64)#ea390d39, c_hist: Float64Array(2)#8bcb3824 at 0 of 16, cB_hist: Float64Array(1000)#28b5b74 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -29.09366424828376, dBfs_max: number -1.6994747766569187, members: number 1, sliceWidth: number 64, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: width 1.5": "{rgba: ArrayBuffer(256)#d9506094, gauge_mins: ArrayBuffer(1)#ca0c003e, gauge_maxs: ArrayBuffer(1)#680b65f8, gauge_amps: ArrayBuffer(1)#7a0b824e, c_hist: Float64Array(2)#48264968 at 0 of 16, cB_hist: Float64Array(1000)#8383dcc5 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -20.80571986754217, dBfs_max: number -2.285438743784166, members: number 1, sliceWidth: number 1, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: channelMode a string": "{rgba: ArrayBuffer(1024)#20c583f4, gauge_mins: ArrayBuffer(4)#4b95f515, gauge_maxs: ArrayBuffer(4)#998c1c65, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#803e9ffe at 0 of 16, cB_hist: Float64Array(1000)#273ff7f5 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -Infinity, dBfs_max: number -4.5389793905405185, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: channelMode undefined": "as well-formed",
        "groupRenderSync: block_norm a string": "{rgba: ArrayBuffer(1024)#c3705c5, gauge_mins: ArrayBuffer(4)#4b95f515, gauge_maxs: ArrayBuffer(4)#4b95f515, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#6604e095 at 0 of 16, cB_hist: Float64Array(1000)#772d4a55 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -Infinity, dBfs_max: number -200, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: block_norm undefined": "{rgba: ArrayBuffer(1024)#c3705c5, gauge_mins: ArrayBuffer(4)#4b95f515, gauge_maxs: ArrayBuffer(4)#4b95f515, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#6604e095 at 0 of 16, cB_hist: Float64Array(1000)#772d4a55 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -Infinity, dBfs_max: number -200, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: gain a string": "{rgba: ArrayBuffer(1024)#d6fdbb64, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#ea0a44d9, c_hist: Float64Array(2)#ca095d46 at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: gain undefined": "{rgba: ArrayBuffer(1024)#d6fdbb64, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#ea0a44d9, c_hist: Float64Array(2)#ca095d46 at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: range a string": "Error status number -4: range must be finite and > 0",
        "groupRenderSync: range undefined": "Error status number -4: range must be finite and > 0",
        "groupRenderSync: n 0": "Error status number -2: Length is not a power of 2",
        "groupRenderSync: width -1": "Error status number -1: width < 0",
        "groupRenderSync: windowc a plain Array": "TypeError status undefined: windowc must be a Float64Array",
        "groupRenderSync: windowc a Float32Array": "TypeError status undefined: windowc must be a Float64Array",
        "groupRenderSync: windowc of 63 values": "RangeError status undefined: windowc is shorter than n",
        "groupRenderSync: buffer missing": "TypeError status undefined: buffer must be an ArrayBuffer",
        "groupRenderSync: buffer a number": "TypeError status undefined: buffer must be an ArrayBuffer",
        "groupRenderSync: lut missing": "TypeError status undefined: lut must be a Uint8Array",
        "groupRenderSync: lut a Uint8ClampedArray": "as well-formed",
        "groupRenderSync: lut of 2 bytes": "Error status number -4: lut_len must be 1..SP_MAX_LUT",
        "groupRenderSync: waterfall undefined": "{rgba: ArrayBuffer(1024)#23263895, gauge_mins: ArrayBuffer(4)#38ecfb93, gauge_maxs: ArrayBuffer(4)#c15d9f6, gauge_amps: ArrayBuffer(4)#e3160fb1, c_hist: Float64Array(2)#7a62ba4a at 0 of 16, cB_hist: Float64Array(1000)#af1b8822 at 0 of 8000, stages: {take_us, native_us}, dBfs_min: number -27.292974425903843, dBfs_max: number -1.9845894562251551, members: number 1, sliceWidth: number 4, transport: string \"none\", transportNote: string, timings: {render_ms, gather_ms, download_ms}}",
        "groupRenderSync: detector 2": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "groupRenderSync: detector 'peak'": "RangeError status undefined: detector must be 0 (sample) or 1 (peak)",
        "renderTracesSync: a group handle": "Error status undefined: renderTraces takes a context handle, not a group",
        "renderIndexSync: a group handle": "Error status undefined: renderIndex takes a context handle, not a group",
        "renderDensitySync: a group handle": "Error status undefined: renderDensity takes a context handle, not a group",
        "renderPowerSync: a group handle": "Error status undefined: renderPower takes a context handle, not a group",
        "renderMeanSync: a group handle": "Error status undefined: renderMean takes a context handle, not a group",
        "renderBandPowerSync: a group handle": "Error status undefined: renderBandPower takes a context handle, not a group",
        "renderTrackSync: a group handle": "Error status undefined: renderTrack takes a context handle, not a group",
        "renderOccupancySync: a group handle": "Error status undefined: renderOccupancy takes a context handle, not a group",
        "renderBatchSync: a group handle": "Error status undefined: renderBatch takes a context handle, not a group",
        "renderTracesSync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderIndexSync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderDensitySync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderPowerSync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderMeanSync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderBandPowerSync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderTrackSync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderOccupancySync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderSync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderNamedSync: a destroyed handle": "Error status undefined: context has been destroyed",
        "renderBatchSync: a destroyed handle": "Error status undefined: context has been destroyed",
        "groupRenderSync: a destroyed handle": "Error status undefined: context has been destroyed",
    },
}

async function main(part, flag) {
    assert.ok(part === 'cpu' || part === 'gpu', 'usage: check_addon_shapes.js <cpu|gpu> [--print]')
    if (part === 'cpu') partA()
    else await partB()
    if (flag === '--print') {
        for (const k of Object.keys(got)) console.log(`        ${JSON.stringify(k)}: ${JSON.stringify(got[k])},`)
        return
    }
    const want = EXPECT[part]
    assert.deepStrictEqual(Object.keys(got), Object.keys(want))
    for (const k of Object.keys(want)) assert.strictEqual(got[k], want[k], k)
    console.log(`addon shapes ok (${part}): ${Object.keys(want).length} cases, ${EXPORTS.length} exports`)
}

main(process.argv[2], process.argv[3]).then(() => process.exit(0), e => { console.error(e.stack || e); process.exit(1) })
