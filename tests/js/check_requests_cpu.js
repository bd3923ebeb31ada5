'use strict'
/**
 * CPU-only: what every request builder of HipWorker makes of one well-formed message and of that message with one field broken at a
 * time, called through HipWorker.prototype - no instance, no GPU - and the addon's export table.  EXPECT holds what the builders did
 * before the Node host was folded into shared pieces, one line per case: the built request's own properties with each value's type and
 * value (bytes as an FNV-1a digest), or the refusal's class, status and message.  `--print` prints the lines of the code as it is.
 */
const assert = require('assert')
const addon = require('../../spectroplot-js_amd/lib/spectroplot_hip.node')
const { HipWorker } = require('../../spectroplot-js_amd/js')

// every name of the addon's Init table
const EXPORTS = ['deviceCount', 'parseFormat', 'window', 'sliceBounds', 'createContext', 'destroyContext', 'allocBuffer', 'poolStats', 'cmap',
    'cmapKeys', 'render', 'renderSync', 'renderNamed', 'renderNamedSync', 'renderBatch', 'renderBatchSync', 'renderTraces', 'renderTracesSync',
    'renderPower', 'renderPowerSync', 'renderMean', 'renderMeanSync', 'bandRows', 'renderBandPower', 'renderBandPowerSync', 'renderTrack',
    'renderTrackSync', 'renderOccupancy', 'renderOccupancySync', 'renderIndex', 'renderIndexSync', 'renderDensity', 'renderDensitySync',
    'namedResolve', 'peakSubframes', 'planCreations', 'createGroup', 'destroyGroup', 'groupRender', 'groupRenderSync']
assert.strictEqual(EXPORTS.length, 40)
for (const k of EXPORTS) assert.strictEqual(typeof addon[k], 'function', k)

function fnv(bytes) {
    let h = 0x811c9dc5
    for (let i = 0; i < bytes.length; i++) h = Math.imul(h ^ bytes[i], 0x01000193) >>> 0
    return h.toString(16)
}
function show(v) {
    if (v instanceof ArrayBuffer) return `ArrayBuffer(${v.byteLength})#${fnv(new Uint8Array(v))}`
    if (ArrayBuffer.isView(v)) return `${v.constructor.name}(${v.length})#${fnv(new Uint8Array(v.buffer, v.byteOffset, v.byteLength))}`
    if (typeof v === 'number' || typeof v === 'boolean') return `${typeof v} ${Object.is(v, -0) ? '-0' : String(v)}`
    if (typeof v === 'string') return `string ${JSON.stringify(v)}`
    return v === null ? 'null' : typeof v === 'undefined' ? 'undefined' : `${typeof v} ${JSON.stringify(v)}`
}
// a refusal as one string, a built request as the list of its properties
function outcome(fn) {
    let r
    try { r = fn() } catch (e) { return `${e.constructor.name} status ${show(e.status)}: ${e.message}` }
    return Object.getOwnPropertyNames(r).map(k => `${k}: ${show(r[k])}`)
}
// ... and its line: in full for the well-formed message, otherwise the properties that differ from the well-formed request's
function line(props, base) {
    if (typeof props === 'string') return props
    if (!base || props.length !== base.length) return '{' + props.join(', ') + '}'
    const differ = props.filter((p, i) => p !== base[i])
    return differ.length ? 'as well-formed but ' + differ.join(', ') : 'as well-formed'
}

const samples = new Uint8Array(1024)
for (let i = 0; i < samples.length; i++) samples[i] = (i * 37 + 11 + (i >> 8) * 5) & 255
// cu8, n = 64, width = 4, 512 bytes, a 2-entry colour map
const message = () => ({ format: 'cu8', n: 64, width: 4, buffer: samples.buffer.slice(0, 512), cmap: [[0, 0, 0], [255, 255, 255]],
    windowc: Float64Array.from({ length: 64 }, (_, i) => 0.5 + i / 128), block_norm: 0.03125, gain: 6, range: 30, channelMode: false,
    waterfall: true, offset: 3, window: 'hann' })
const options = () => ({ db: true, bands: [[0, 8], [8, 64]] })

const set = (k, v) => m => { m[k] = v }
const BREAKS = [
    ['well-formed', () => {}],
    ['buffer missing', m => { delete m.buffer }],
    ['buffer a number', set('buffer', 7)],
    ['buffer a view at byteOffset 256', set('buffer', new Uint8Array(samples.buffer, 256, 512))],
    ["detector 'peak'", set('detector', 'peak')],
    ["detector 'rms'", set('detector', 'rms')],
    ['detector 2', set('detector', 2)],
    ["cmap a string", set('cmap', 'viridis')],
    ['windowc a plain Array', m => { m.windowc = Array.from(m.windowc) }],
]
for (const k of ['n', 'width', 'gain', 'range', 'block_norm']) BREAKS.push([`${k} a string`, set(k, '12')], [`${k} undefined`, set(k, undefined)])
const BAND_BREAKS = [
    ['no options', () => undefined],
    ['db absent, flat Int32Array', () => ({ bands: Int32Array.from([0, 8, 8, 64]) })],
    ['bands missing', () => ({ db: true })],
    ['bands of odd length', () => ({ bands: [0, 1, 2] })],
    ['65 pairs', () => ({ bands: new Array(65).fill([0, 1]) })],
    ['y1 > n', () => ({ bands: [[0, 65]] })],
    ['y0 > y1', () => ({ bands: [[5, 4]] })],
    ['fractional', () => ({ bands: [[0, 1.5]] })],
]
const BUILDERS = ['_request', '_namedRequest', '_tracesRequest', '_powerRequest', '_meanRequest', '_bandRequest', '_indexRequest']

const got = {}
for (const b of BUILDERS) {
    assert.strictEqual(typeof HipWorker.prototype[b], 'function', b)
    const base = outcome(() => HipWorker.prototype[b](message(), options()))
    for (const [name, brk] of BREAKS) {
        const m = message()
        brk(m)
        got[`${b}: ${name}`] = line(outcome(() => HipWorker.prototype[b](m, options())), name === 'well-formed' ? null : base)
    }
    if (['_powerRequest', '_meanRequest', '_bandRequest'].includes(b))
        for (const [name, opt] of BAND_BREAKS) got[`${b} options: ${name}`] = line(outcome(() => HipWorker.prototype[b](message(), opt())), base)
    // (_request and _namedRequest read the message's fields unasked)
    if (BUILDERS.indexOf(b) >= 2) got[`${b}: no message`] = line(outcome(() => HipWorker.prototype[b](undefined, options())), base)
}

const EXPECT = {
    "_request: well-formed": "{format: number 2, buffer: ArrayBuffer(512)#1316acc5, n: number 64, windowc: Float64Array(64)#b521b405, block_norm: number 0.03125, gain: number 6, range: number 30, lut: Uint8Array(6)#293250ee, width: number 4, channelMode: boolean false, waterfall: boolean true, detector: number 0}",
    "_request: buffer missing": "as well-formed but buffer: undefined",
    "_request: buffer a number": "as well-formed but buffer: number 7",
    "_request: buffer a view at byteOffset 256": "as well-formed but buffer: ArrayBuffer(512)#35e740c5",
    "_request: detector 'peak'": "as well-formed but detector: number 1",
    "_request: detector 'rms'": "Error status number -1: detector must be 'sample' or 'peak', not \"rms\"",
    "_request: detector 2": "Error status number -1: detector must be 'sample' or 'peak', not 2",
    "_request: cmap a string": "as well-formed but lut: Uint8Array(21)#214171cf",
    "_request: windowc a plain Array": "as well-formed",
    "_request: n a string": "as well-formed but n: string \"12\"",
    "_request: n undefined": "as well-formed but n: undefined",
    "_request: width a string": "as well-formed but width: string \"12\"",
    "_request: width undefined": "as well-formed but width: undefined",
    "_request: gain a string": "as well-formed but gain: string \"12\"",
    "_request: gain undefined": "as well-formed but gain: undefined",
    "_request: range a string": "as well-formed but range: string \"12\"",
    "_request: range undefined": "as well-formed but range: undefined",
    "_request: block_norm a string": "as well-formed but block_norm: string \"12\"",
    "_request: block_norm undefined": "as well-formed but block_norm: undefined",
    "_namedRequest: well-formed": "{format: string \"cu8\", window: string \"hann\", cmap: string \"0,0,0,255,255,255\", buffer: ArrayBuffer(512)#1316acc5, n: number 64, width: number 4, gain: number 6, range: number 30, channelMode: boolean false, waterfall: boolean true, detector: number 0}",
    "_namedRequest: buffer missing": "as well-formed but buffer: undefined",
    "_namedRequest: buffer a number": "as well-formed but buffer: number 7",
    "_namedRequest: buffer a view at byteOffset 256": "as well-formed but buffer: ArrayBuffer(512)#35e740c5",
    "_namedRequest: detector 'peak'": "as well-formed but detector: number 1",
    "_namedRequest: detector 'rms'": "Error status number -1: detector must be 'sample' or 'peak', not \"rms\"",
    "_namedRequest: detector 2": "Error status number -1: detector must be 'sample' or 'peak', not 2",
    "_namedRequest: cmap a string": "as well-formed but cmap: string \"viridis\"",
    "_namedRequest: windowc a plain Array": "as well-formed",
    "_namedRequest: n a string": "as well-formed but n: string \"12\"",
    "_namedRequest: n undefined": "as well-formed but n: undefined",
    "_namedRequest: width a string": "as well-formed but width: string \"12\"",
    "_namedRequest: width undefined": "as well-formed but width: undefined",
    "_namedRequest: gain a string": "as well-formed but gain: string \"12\"",
    "_namedRequest: gain undefined": "as well-formed",
    "_namedRequest: range a string": "as well-formed but range: string \"12\"",
    "_namedRequest: range undefined": "as well-formed",
    "_namedRequest: block_norm a string": "as well-formed",
    "_namedRequest: block_norm undefined": "as well-formed",
    "_tracesRequest: well-formed": "{format: number 2, buffer: ArrayBuffer(512)#1316acc5, n: number 64, windowc: Float64Array(64)#b521b405, block_norm: number 0.03125, gain: number 6, range: number 30, width: number 4, channelMode: boolean false}",
    "_tracesRequest: buffer missing": "Error status number -1: a traces request needs a buffer",
    "_tracesRequest: buffer a number": "as well-formed but buffer: number 7",
    "_tracesRequest: buffer a view at byteOffset 256": "as well-formed but buffer: ArrayBuffer(512)#35e740c5",
    "_tracesRequest: detector 'peak'": "Error status number -4: traces of the peak detector are not supported",
    "_tracesRequest: detector 'rms'": "Error status number -1: detector must be 'sample' or 'peak', not \"rms\"",
    "_tracesRequest: detector 2": "Error status number -1: detector must be 'sample' or 'peak', not 2",
    "_tracesRequest: cmap a string": "as well-formed",
    "_tracesRequest: windowc a plain Array": "as well-formed",
    "_tracesRequest: n a string": "as well-formed but n: string \"12\"",
    "_tracesRequest: n undefined": "as well-formed but n: undefined",
    "_tracesRequest: width a string": "as well-formed but width: string \"12\"",
    "_tracesRequest: width undefined": "as well-formed but width: undefined",
    "_tracesRequest: gain a string": "as well-formed but gain: string \"12\"",
    "_tracesRequest: gain undefined": "as well-formed but gain: undefined",
    "_tracesRequest: range a string": "as well-formed but range: string \"12\"",
    "_tracesRequest: range undefined": "as well-formed but range: undefined",
    "_tracesRequest: block_norm a string": "as well-formed but block_norm: string \"12\"",
    "_tracesRequest: block_norm undefined": "as well-formed but block_norm: undefined",
    "_tracesRequest: no message": "Error status number -1: a traces request needs a buffer",
    "_powerRequest: well-formed": "{format: number 2, buffer: ArrayBuffer(512)#1316acc5, n: number 64, windowc: Float64Array(64)#b521b405, block_norm: number 0.03125, gain: number 6, range: number 30, width: number 4, channelMode: boolean false, db: boolean true}",
    "_powerRequest: buffer missing": "Error status number -1: a power request needs a buffer",
    "_powerRequest: buffer a number": "as well-formed but buffer: number 7",
    "_powerRequest: buffer a view at byteOffset 256": "as well-formed but buffer: ArrayBuffer(512)#35e740c5",
    "_powerRequest: detector 'peak'": "Error status number -4: the power plane of the peak detector is not supported",
    "_powerRequest: detector 'rms'": "Error status number -1: detector must be 'sample' or 'peak', not \"rms\"",
    "_powerRequest: detector 2": "Error status number -1: detector must be 'sample' or 'peak', not 2",
    "_powerRequest: cmap a string": "as well-formed",
    "_powerRequest: windowc a plain Array": "as well-formed",
    "_powerRequest: n a string": "as well-formed but n: string \"12\"",
    "_powerRequest: n undefined": "as well-formed but n: undefined",
    "_powerRequest: width a string": "as well-formed but width: string \"12\"",
    "_powerRequest: width undefined": "as well-formed but width: undefined",
    "_powerRequest: gain a string": "as well-formed but gain: string \"12\"",
    "_powerRequest: gain undefined": "as well-formed but gain: undefined",
    "_powerRequest: range a string": "as well-formed but range: string \"12\"",
    "_powerRequest: range undefined": "as well-formed but range: undefined",
    "_powerRequest: block_norm a string": "as well-formed but block_norm: string \"12\"",
    "_powerRequest: block_norm undefined": "as well-formed but block_norm: undefined",
    "_powerRequest options: no options": "as well-formed but db: boolean false",
    "_powerRequest options: db absent, flat Int32Array": "as well-formed but db: boolean false",
    "_powerRequest options: bands missing": "as well-formed",
    "_powerRequest options: bands of odd length": "as well-formed but db: boolean false",
    "_powerRequest options: 65 pairs": "as well-formed but db: boolean false",
    "_powerRequest options: y1 > n": "as well-formed but db: boolean false",
    "_powerRequest options: y0 > y1": "as well-formed but db: boolean false",
    "_powerRequest options: fractional": "as well-formed but db: boolean false",
    "_powerRequest: no message": "Error status number -1: a power request needs a buffer",
    "_meanRequest: well-formed": "{format: number 2, buffer: ArrayBuffer(512)#1316acc5, n: number 64, windowc: Float64Array(64)#b521b405, block_norm: number 0.03125, gain: number 6, range: number 30, width: number 4, channelMode: boolean false, db: boolean true}",
    "_meanRequest: buffer missing": "Error status number -1: a mean request needs a buffer",
    "_meanRequest: buffer a number": "as well-formed but buffer: number 7",
    "_meanRequest: buffer a view at byteOffset 256": "as well-formed but buffer: ArrayBuffer(512)#35e740c5",
    "_meanRequest: detector 'peak'": "Error status number -4: the mean power of the peak detector is not supported",
    "_meanRequest: detector 'rms'": "Error status number -1: detector must be 'sample' or 'peak', not \"rms\"",
    "_meanRequest: detector 2": "Error status number -1: detector must be 'sample' or 'peak', not 2",
    "_meanRequest: cmap a string": "as well-formed",
    "_meanRequest: windowc a plain Array": "as well-formed",
    "_meanRequest: n a string": "as well-formed but n: string \"12\"",
    "_meanRequest: n undefined": "as well-formed but n: undefined",
    "_meanRequest: width a string": "as well-formed but width: string \"12\"",
    "_meanRequest: width undefined": "as well-formed but width: undefined",
    "_meanRequest: gain a string": "as well-formed but gain: string \"12\"",
    "_meanRequest: gain undefined": "as well-formed but gain: undefined",
    "_meanRequest: range a string": "as well-formed but range: string \"12\"",
    "_meanRequest: range undefined": "as well-formed but range: undefined",
    "_meanRequest: block_norm a string": "as well-formed but block_norm: string \"12\"",
    "_meanRequest: block_norm undefined": "as well-formed but block_norm: undefined",
    "_meanRequest options: no options": "as well-formed but db: boolean false",
    "_meanRequest options: db absent, flat Int32Array": "as well-formed but db: boolean false",
    "_meanRequest options: bands missing": "as well-formed",
    "_meanRequest options: bands of odd length": "as well-formed but db: boolean false",
    "_meanRequest options: 65 pairs": "as well-formed but db: boolean false",
    "_meanRequest options: y1 > n": "as well-formed but db: boolean false",
    "_meanRequest options: y0 > y1": "as well-formed but db: boolean false",
    "_meanRequest options: fractional": "as well-formed but db: boolean false",
    "_meanRequest: no message": "Error status number -1: a mean request needs a buffer",
    "_bandRequest: well-formed": "{format: number 2, buffer: ArrayBuffer(512)#1316acc5, n: number 64, windowc: Float64Array(64)#b521b405, block_norm: number 0.03125, gain: number 6, range: number 30, width: number 4, channelMode: boolean false, db: boolean true, bands: Int32Array(4)#25d165c5}",
    "_bandRequest: buffer missing": "Error status number -1: a band-power request needs a buffer",
    "_bandRequest: buffer a number": "as well-formed but buffer: number 7",
    "_bandRequest: buffer a view at byteOffset 256": "as well-formed but buffer: ArrayBuffer(512)#35e740c5",
    "_bandRequest: detector 'peak'": "Error status number -4: the band power of the peak detector is not supported",
    "_bandRequest: detector 'rms'": "Error status number -1: detector must be 'sample' or 'peak', not \"rms\"",
    "_bandRequest: detector 2": "Error status number -1: detector must be 'sample' or 'peak', not 2",
    "_bandRequest: cmap a string": "as well-formed",
    "_bandRequest: windowc a plain Array": "as well-formed",
    "_bandRequest: n a string": "Error status number -1: a band must satisfy 0 <= y0 <= y1 <= n",
    "_bandRequest: n undefined": "as well-formed but n: undefined",
    "_bandRequest: width a string": "as well-formed but width: string \"12\"",
    "_bandRequest: width undefined": "as well-formed but width: undefined",
    "_bandRequest: gain a string": "as well-formed but gain: string \"12\"",
    "_bandRequest: gain undefined": "as well-formed but gain: undefined",
    "_bandRequest: range a string": "as well-formed but range: string \"12\"",
    "_bandRequest: range undefined": "as well-formed but range: undefined",
    "_bandRequest: block_norm a string": "as well-formed but block_norm: string \"12\"",
    "_bandRequest: block_norm undefined": "as well-formed but block_norm: undefined",
    "_bandRequest options: no options": "Error status number -1: a band-power request needs {bands}: [y0, y1] pairs",
    "_bandRequest options: db absent, flat Int32Array": "as well-formed but db: boolean false",
    "_bandRequest options: bands missing": "Error status number -1: a band-power request needs {bands}: [y0, y1] pairs",
    "_bandRequest options: bands of odd length": "Error status number -1: bands must be at most 64 [y0, y1] pairs",
    "_bandRequest options: 65 pairs": "Error status number -1: bands must be at most 64 [y0, y1] pairs",
    "_bandRequest options: y1 > n": "Error status number -1: a band must satisfy 0 <= y0 <= y1 <= n",
    "_bandRequest options: y0 > y1": "Error status number -1: a band must satisfy 0 <= y0 <= y1 <= n",
    "_bandRequest options: fractional": "Error status number -1: a band must satisfy 0 <= y0 <= y1 <= n",
    "_bandRequest: no message": "Error status number -1: a band-power request needs a buffer",
    "_indexRequest: well-formed": "{format: number 2, buffer: ArrayBuffer(512)#1316acc5, n: number 64, windowc: Float64Array(64)#b521b405, block_norm: number 0.03125, gain: number 6, range: number 30, lut: Uint8Array(6)#293250ee, width: number 4, channelMode: boolean false, waterfall: boolean true, detector: number 0}",
    "_indexRequest: buffer missing": "Error status number -1: an indexed request needs a buffer",
    "_indexRequest: buffer a number": "as well-formed but buffer: number 7",
    "_indexRequest: buffer a view at byteOffset 256": "as well-formed but buffer: ArrayBuffer(512)#35e740c5",
    "_indexRequest: detector 'peak'": "as well-formed but detector: number 1",
    "_indexRequest: detector 'rms'": "Error status number -1: detector must be 'sample' or 'peak', not \"rms\"",
    "_indexRequest: detector 2": "Error status number -1: detector must be 'sample' or 'peak', not 2",
    "_indexRequest: cmap a string": "Error status number -1: an indexed request needs a colour map",
    "_indexRequest: windowc a plain Array": "as well-formed",
    "_indexRequest: n a string": "Error status number -1: n must be a number, not \"12\"",
    "_indexRequest: n undefined": "Error status number -1: n must be a number, not undefined",
    "_indexRequest: width a string": "Error status number -1: width must be a number, not \"12\"",
    "_indexRequest: width undefined": "Error status number -1: width must be a number, not undefined",
    "_indexRequest: gain a string": "Error status number -1: gain must be a number, not \"12\"",
    "_indexRequest: gain undefined": "Error status number -1: gain must be a number, not undefined",
    "_indexRequest: range a string": "Error status number -1: range must be a number, not \"12\"",
    "_indexRequest: range undefined": "Error status number -1: range must be a number, not undefined",
    "_indexRequest: block_norm a string": "Error status number -1: block_norm must be a number, not \"12\"",
    "_indexRequest: block_norm undefined": "Error status number -1: block_norm must be a number, not undefined",
    "_indexRequest: no message": "Error status number -1: an indexed request needs a buffer",
}

if (process.argv[2] === '--print') {
    for (const k of Object.keys(got)) console.log(`    ${JSON.stringify(k)}: ${JSON.stringify(got[k])},`)
    process.exit(0)
}
assert.deepStrictEqual(Object.keys(got), Object.keys(EXPECT))
for (const k of Object.keys(EXPECT)) assert.strictEqual(got[k], EXPECT[k], k)
console.log(`request builders ok: ${Object.keys(EXPECT).length} cases, ${EXPORTS.length} exports`)
