'use strict'
/**
 * CPU: js/consumers.js `recolour` against fixtures pytest has written into argv[2] (tests/test_index_cpu.py): index.bin, and per colour
 * map of tests/golden/cmaps.bin <name>.rgba = numpy's take of the map (alpha 255; an index the map does not have: 0, 0, 0, 255).  The map
 * is passed as the reference's array of [r, g, b] entries and as a packed Uint8Array, whole and cut to 100 entries.
 */
const fs = require('fs')
const path = require('path')
const { recolour } = require('../../spectroplot-js_amd/js/consumers.js')

const dir = process.argv[2]
const gdir = path.join(__dirname, '..', 'golden')
const meta = JSON.parse(fs.readFileSync(path.join(gdir, 'cmaps.json'), 'utf8'))
const bin = fs.readFileSync(path.join(gdir, 'cmaps.bin'))
const index = new Uint8Array(fs.readFileSync(path.join(dir, 'index.bin')))
let checked = 0
for (const e of meta) {
    for (const len of [e.length, 100]) {
        const packed = new Uint8Array(bin.buffer, bin.byteOffset + e.offset, 3 * len)
        const entries = []
        for (let i = 0; i < len; i++) entries.push([packed[3 * i], packed[3 * i + 1], packed[3 * i + 2]])
        const want = fs.readFileSync(path.join(dir, `${e.name}_${len}.rgba`))
        for (const [how, cmap] of [['entries', entries], ['packed', packed]]) {
            const got = recolour(index, cmap)
            if (!(got instanceof Uint8ClampedArray) || got.length !== 4 * index.length) throw new Error(`${e.name} ${how}: shape`)
            if (Buffer.compare(Buffer.from(got.buffer), want) !== 0) throw new Error(`${e.name} ${len} ${how}: bytes differ`)
            checked++
        }
    }
}
if (recolour(new Uint8Array(0), [[1, 2, 3]]).length !== 0) throw new Error('empty image')
console.log(`recolour checks ok: ${checked}`)
