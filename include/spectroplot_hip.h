/*
 * spectroplot_hip.h — C ABI of the MI355X-native I/Q STFT -> RGBA hot path.
 *
 * This library replaces the compute half of triq-org/spectroplot-js' Web Worker (lib/worker.js `renderFft`):
 * sample decode -> taper -> radix-2 DFT -> |X|^2 -> dB -> colour index -> RGBA, plus the worker's side outputs
 * (two histograms, dBfs min/max, three per-frame gauges).  One `sp_context` corresponds to one reference Worker
 * instance (lib/spectroplot.js:85-116): it owns one HIP stream on one device and processes requests in order.
 *
 * Reference interface each entry point replaces (file:line relative to the reference checkout):
 *
 *   sp_format_parse          lib/samples.js:22-162      the format-name table (aliases, unknown -> CU8)
 *   sp_slice_bounds          lib/samples.js:253-258     SampleView.slice: the caller's per-worker byte range
 *   sp_window                lib/windows.js:14-88       named taper generators (optional sugar; the wire carries arrays)
 *   sp_cmap, sp_cmap_key     lib/cube1cmap.js, lib/matplotlibcmaps.js, lib/parabolacmap.js (tables), lib/utils.js:25-40
 *   sp_cmap_generate         lib/soxcmap.js:12-49, lib/naivecmap.js:13-81   the computed maps, evaluated (sp_cmap serves them from here)
 *   sp_render_named          lib/spectroplot.js:1113-1146, 1213-1226   the caller's message assembly from option names
 *   sp_named_resolve         lib/spectroplot.js:238-264, lib/utils.js:25-40   option name -> generator / table entry, with the defaults
 *   sp_twiddles              lib/fft_nayuki.js:42-47    cos/sin tables (exposed for tests)
 *   sp_plan_create           lib/worker.js:30-62        per-request constants + the cached FFT object
 *   sp_render                lib/worker.js:23-156       renderFft(ctx) on host buffers = one postMessage -> one reply
 *   sp_render_strip          lib/worker.js:23-156 + lib/spectroplot.js:1241-1244   the same, written into the strip's band of the caller's image
 *   sp_plan_execute          lib/worker.js:68-137       the frame loop, operands resident in HBM (benchmarks, multi-GPU)
 *   sp_plan_execute_from_host  lib/worker.js:68-137     the same with the capture in host memory (uploaded in chunks under the renders),
 *                                                        outputs resident in HBM: what a group member does with its slice
 *   sp_plan_execute_batch    lib/worker.js:68-137 per item   many captures' frame loops with one plan in one launch, operands in HBM
 *   sp_render_batch          lib/worker.js:23-156 per item + lib/easy.js:22-72 / lib/spectroplot.js:85-116   many instances' requests
 *                                                        queued on one worker pool (one Spectroplot per dropped file), on host buffers
 *   sp_debug_batch_plan      (none)                     (tests) the host's work list for a batch
 *   sp_plan_debug_launch     (none)                     (tests) the launch sp_plan_execute would make for a request
 *   sp_debug_frames_launch   (none)                     (tests) the frame-loop kernels' launch rule alone
 *   sp_debug_scratch_launch  (none)                     (tests) the scratch kernels' launch shape alone
 *   sp_context_debug_set_cu_count  (none)               (tests) the CU count a context's launches are shaped by
 *   sp_merge_replies(_batch) lib/spectroplot.js:1229-1238   the caller's merge of the slices' histograms and dBfs range, on the device
 *   sp_place_strips          lib/spectroplot.js:1241-1244   the caller's putImageData of every slice's strip, on the device
 *   sp_group_render          lib/spectroplot.js:1206-1244, lib/samples.js:253-258   the caller's sliced render: one slice per device, the
 *                                                        strips gathered device to device (RCCL / peer copies), merged on the root
 *   sp_plan_execute_index, sp_render_index   lib/worker.js:105-117   the same renders with the colour index per pixel, not its RGBA
 *   sp_index_to_rgba         lib/worker.js:117-120      the LUT step alone, on an index image
 *   sp_plan_execute_density, sp_render_density, sp_density_from_index   lib/worker.js:105-117   how often each row showed each colour
 *                                                        index: the persistence spectrum of a request, or of an index image
 *   sp_synth_*               (none)                     device-side synthetic I/Q for benchmarks
 *
 * The request fields are the reference message's (lib/spectroplot.js:1213-1226):
 *   block_norm, gain, range, cmap -> lut_rgb/lut_len, n, windowc, width, buffer -> bytes/nbytes, format, channelMode,
 *   waterfall; `offset` is only echoed by the worker and stays in the host wrapper.
 * The reply fields are the reference reply's (lib/worker.js:140-155):
 *   cB_hist[1000], c_hist[lut_len], dBfs_min, dBfs_max, gauge_mins/maxs/amps[width], imageData.data[4*width*n].
 *
 * Numerics: the DFT runs in IEEE f64 with the reference's exact butterfly graph and operation order (no FMA
 * contraction), so |X|^2 is bit-identical to the reference's; colour and histogram indices are taken from exact
 * threshold tables built on the host with a restatement of the engine's Math.log10.  There is no CPU fallback:
 * without a HIP device every compute entry point returns SP_ERR_NO_DEVICE.
 *
 * All functions return SP_OK (0) or a negative status; sp_last_error(ctx) gives a message for the last failure on ctx.
 */
#ifndef SPECTROPLOT_HIP_H
#define SPECTROPLOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_VERSION 100          /* 0.1.0 */
#define SP_CB_HIST_SIZE 1000    /* centi-bel histogram bins, lib/worker.js:41 */
#define SP_MAX_LUT 4096         /* largest colour map accepted */
#define SP_MAX_N (1 << 20)      /* largest FFT length accepted */

enum sp_status {
    SP_OK = 0,
    SP_ERR_INVALID_ARG = -1,
    SP_ERR_NOT_POW2 = -2,        /* reference: throw 'Length is not a power of 2' (lib/fft_nayuki.js:38-39) */
    SP_ERR_BYTE_LENGTH = -3,     /* reference: RangeError, byte length not a multiple of the view's element size */
    SP_ERR_UNSUPPORTED = -4,     /* valid for the reference but outside this library's limits (documented per call) */
    SP_ERR_NO_DEVICE = -5,
    SP_ERR_HIP = -6,
    SP_ERR_NOMEM = -7
};

/* sample formats, lib/samples.js:30-155 */
enum sp_format {
    SP_FMT_CU4 = 0, SP_FMT_CS4, SP_FMT_CU8, SP_FMT_CS8, SP_FMT_CU12, SP_FMT_CS12, SP_FMT_CU16, SP_FMT_CS16,
    SP_FMT_CU32, SP_FMT_CS32, SP_FMT_CU64, SP_FMT_CS64, SP_FMT_CF32, SP_FMT_CF64, SP_FMT_COUNT
};

/*
 * What a column of a sparse request shows (stride = (sampleCount - n) / (width - 1) of lib/worker.js:50 at 2n or more).
 * SP_DETECTOR_SAMPLE is the reference: the column's one frame, the samples up to the next column's frame are skipped (worker.js:68-75).
 * SP_DETECTOR_PEAK is a spectrum analyser's max hold: with M = floor(stride / n) (M = 1 unless width >= 2 and stride is finite and
 * >= 2n), sub-frame j < M of column x starts j * n samples behind the column's frame p(x) = ~~(0.5 + stride * x) and exists if j == 0 or
 * p(x) + (j + 1) * n <= sampleCount; every existing sub-frame is tapered, transformed and split like a frame, and per bin the column keeps
 * the largest |X|^2 of them in order of j (a NaN only if every sub-frame gives NaN: v_max_f64 / fmax).  From that value on the column is
 * the reference's (worker.js:93-136): colour index, both histograms (one count per pixel), dBfs range, gauge_mins / gauge_maxs;
 * gauge_amps stays the centre sample of sub-frame 0.  A request with M == 1 is the sample detector, byte for byte and kernel for kernel.
 * The detector is part of a plan.  Peak plans run through sp_plan_execute, sp_plan_execute_from_host, sp_render, sp_render_strip and
 * sp_render_named_ex; batches and groups (sp_plan_execute_batch, sp_render_batch, sp_group_render(_ex)) return SP_ERR_UNSUPPORTED.
 */
enum sp_detector { SP_DETECTOR_SAMPLE = 0, SP_DETECTOR_PEAK = 1 };

typedef struct sp_context sp_context;
typedef struct sp_plan sp_plan;

/* One render request minus the sample buffer (the reference message, lib/spectroplot.js:1213-1226). Host pointers. */
typedef struct sp_request {
    int32_t format;          /* enum sp_format */
    int32_t n;               /* FFT length, power of two, 2 .. SP_MAX_N */
    int32_t channel_mode;    /* 0 = I/Q, 1 = L/R split (lib/fft_nayuki.js:103-119) */
    int32_t waterfall;       /* 0 = spectrogram (n rows x width cols), 1 = waterfall (width rows x n cols) */
    int32_t lut_len;         /* colour map entries, 1 .. SP_MAX_LUT */
    int32_t detector;        /* enum sp_detector: 0 = sample (the reference: a column shows one frame), 1 = peak hold (below) */
    double block_norm;       /* 1 / sum(taper) */
    double gain;             /* dB */
    double range;            /* dB, finite and > 0 */
    const double *windowc;   /* [n] evaluated taper */
    const uint8_t *lut_rgb;  /* [3 * lut_len] r,g,b per entry (ends already forced by the caller if wanted) */
} sp_request;

/* Reply buffers.  For sp_render these are host pointers, for sp_plan_execute device pointers. Any may be NULL. */
typedef struct sp_reply {
    uint8_t *rgba;           /* [4 * width * n] */
    uint8_t *gauge_mins;     /* [width] */
    uint8_t *gauge_maxs;     /* [width] */
    uint8_t *gauge_amps;     /* [width] */
    uint64_t *c_hist;        /* [lut_len]  overwritten with the counts of this request */
    uint64_t *cb_hist;       /* [SP_CB_HIST_SIZE]  likewise */
    double *dbfs_minmax;     /* [2] = {dBfs_min, dBfs_max} */
} sp_reply;

int sp_version(void);
const char *sp_status_string(int status);
const char *sp_last_error(const sp_context *ctx);

/* ---- pure host helpers (no device needed) ------------------------------------------------------------- */

/* Maps a format name (any case, aliases, unknown -> CU8) to its id and bytes per complex sample. */
int sp_format_parse(const char *name, int32_t *format, int32_t *sample_width);
/* Element size of the typed view the reference lays over the buffer (byte length must be a multiple of it). */
int sp_format_element_size(int32_t format);
/* The caller's slice `index` of `count` over a capture of `nbytes` bytes: [*begin, *end) in bytes. */
int sp_slice_bounds(size_t nbytes, int32_t sample_width, int32_t index, int32_t count, size_t *begin, size_t *end);
/* Named tapers: "rectangular", "bartlett", "hamming", "hann", "blackman", "blackmanHarris" (exact names). */
int sp_window(const char *name, int32_t n, double *window, double *weight);
/*
 * Colour maps of the reference under its own keys ("cube1_cmap", "sox_cmap", ... "viridis_cmap", "parabola_cmap"), in the key
 * order of its merged table (lib/spectroplot.js:41).  sp_cmap resolves `name` as lib/utils.js:25-40 does (exact, then
 * case-insensitive, then case-insensitive prefix, first hit in key order) and copies the r,g,b triples as the reference's
 * modules evaluate them, i.e. BEFORE the caller's end forcing (lib/spectroplot.js:1129-1130).  *lut_len receives the entry count
 * (also when rgb is NULL or capacity_entries is too small, which returns SP_ERR_INVALID_ARG); an unknown name returns
 * SP_ERR_UNSUPPORTED.
 */
int sp_cmap_count(void);
const char *sp_cmap_key(int32_t index);
int sp_cmap(const char *name, uint8_t *rgb, int32_t capacity_entries, int32_t *lut_len);
/*
 * The reference's computed colour maps as the functions they are (lib/soxcmap.js:12-49 `sox_cmap`; lib/naivecmap.js:13-81 `naive_cmap`,
 * `grayscale_cmap`, `roentgen_cmap`, `phosphor_cmap`): `stops` entries (the reference exports them at 256) of r, g, b into rgb[3 * stops].
 * sp_cmap serves these five from the same generators; SP_ERR_UNSUPPORTED for any other key (the other maps are literal tables there too).
 */
int sp_cmap_generate(const char *key, int32_t stops, uint8_t *rgb);
/* cosTable / sinTable of the reference's FFT object, n/2 entries each. */
int sp_twiddles(int32_t n, double *cos_table, double *sin_table);
/* The engine's Math.log10 as restated by this library (exposed so tests can pin it). */
double sp_js_log10(double x);
/*
 * The peak detector's sub-frame rule for a request of this shape (enum sp_detector): *subframes = M, the sub-frames per column (1: the
 * request is the sample detector's), *last_column_count = how many of them exist in column width - 1 (every other column has all M
 * whenever M >= 2).  width 0 gives (1, 0).  Either output may be NULL.
 */
int sp_peak_subframes(int32_t format, int32_t n, size_t nbytes, int32_t width, int32_t *subframes, int32_t *last_column_count);

/* ---- device ------------------------------------------------------------------------------------------- */

int sp_device_count(int32_t *count);
/* One context = one reference Worker: one device, one stream, in-order execution. */
int sp_context_create(int32_t device, sp_context **ctx);
void sp_context_destroy(sp_context *ctx);
/* Uses an existing hipStream_t instead of the context's own (e.g. the caller's framework stream). NULL restores. */
int sp_context_set_stream(sp_context *ctx, void *hip_stream);
/* The stream a caller bound with sp_context_set_stream, NULL while the context uses its own (what to hand back to set_stream to restore). */
int sp_context_get_stream(const sp_context *ctx, void **hip_stream);
int sp_context_synchronize(sp_context *ctx);

/*
 * renderFft on host buffers: copies `bytes` to the device, renders, copies the reply back, synchronously.
 * Plans are cached inside the context while n / taper / LUT / gain / range / block_norm stay the same, as the
 * reference caches its FFT object (lib/worker.js:59-62).
 */
int sp_render(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply);
/*
 * The same render delivered where the caller's merge would put it (lib/spectroplot.js:1241-1244, putImageData(strip, offset, 0)):
 * reply->rgba points at the strip's first pixel INSIDE an image of image_width >= width frames - spectrogram layout: column `offset` of
 * row 0, rows 4 * image_width bytes apart; waterfall layout: the first of the strip's `width` contiguous rows.  Everything else as
 * sp_render (sp_render is sp_render_strip with image_width = width).
 */
int sp_render_strip(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply,
                    int32_t image_width);
/*
 * Bytes of samples the last sp_render / sp_render_strip / sp_render_named on this context sent over the host link.  A request whose
 * frames are more than n samples apart (stride > n, lib/worker.js:50: the reference's loop skips the samples in between, :70-75) and lie
 * inside the capture uploads the frames' own samples only, as rows of pitched copies into a packed device buffer; every other request
 * uploads the capture as it is.  SPECTROPLOT_HIP_NO_PACKED_UPLOAD=1 turns the packed upload off.
 * A large request (>= 16 MiB of samples + image, width >= 1024) is pipelined in chunks of frames: 4, from 64 MiB 6, of UNEVEN size -
 * each 0.65 of its neighbour, shrinking towards the end of the longer transfer's direction.
 */
int sp_context_last_upload_bytes(const sp_context *ctx, size_t *nbytes);
/* (tests) In how many chunks of frames the streamer carried that request out (1: everything on the context's stream, nothing
 * overlapped); sp_debug_upload_plan sizes a request's image at 4 bytes per pixel and cannot describe an indexed one. */
int sp_context_last_chunks(const sp_context *ctx, int32_t *chunks);
/*
 * (tests) The upload plan sp_render would follow for a request of this shape, without a device: how [0, width) is cut into chunks of
 * frames and, for a sparse request, the packed layout and the pitched copies of every chunk.  out[] receives int64 words: packed (0 / 1),
 * chunks, device bytes, link bytes; per chunk x0, x1 and, if packed: the capture's sample where frame x0 starts, the samples between
 * source rows (floor(stride)) and between device rows, the chunk's byte offset on the device, the kernel's position of frames x0 and
 * x1 - 1, the bit pattern of the kernel's stride, the number of pitched copies, then first row, end row, smallest and largest drift
 * per copy.  *used = words needed (SP_ERR_INVALID_ARG if capacity is smaller).  tests/test_upload_plan_cpu.py checks every frame of
 * thousands of shapes against the reference's own positions (lib/worker.js:72).
 */
int sp_debug_upload_plan(int32_t format, int32_t n, size_t nbytes, int32_t width, int32_t want_image, int64_t *out, size_t capacity,
                         size_t *used);
/*
 * (tests) Where a sliced render of `count` workers puts its strips in the caller's image (lib/spectroplot.js:1208, 1244), without a
 * device: the layout sp_group_render_ex follows with either gather.  Bands and the un-drawn rest are rectangles of bytes in the RGBA
 * image: `rows` rows of `row bytes`, `pitch` bytes apart.  out[] receives int64 words: slice width, strip bytes, rest (frames no strip
 * draws), the bands' pitch, row bytes and rows, the rest's offset, pitch, row bytes and rows; then per strip the byte offset of its band
 * and the offset of its gauges.  *used = words needed (SP_ERR_INVALID_ARG if capacity is smaller).  tests/test_slice_layout_cpu.py
 * checks it against the reference's formulas.
 */
int sp_debug_slice_layout(int32_t n, int32_t width, int32_t count, int32_t waterfall, int64_t *out, size_t capacity, size_t *used);

/*
 * The same with the request given by names, as the reference's caller assembles its message from options
 * (lib/spectroplot.js:1113-1146): window = lookup(windows, name) or blackmanHarris, block_norm = 1 / weight, cmap = lookup or
 * cube1 with its ends forced to black / white, format by sp_format_parse.  The plan (and its device tables) is kept while the
 * names and numbers repeat: nothing is re-evaluated or re-uploaded then.
 */
typedef struct sp_named_request {
    const char *format;      /* "cu8", "CF32", ... (unknown -> CU8, as the reference) */
    const char *window;      /* "hann", "blackmanHarris", ... (lookup rules of lib/utils.js:25-40; no hit -> blackmanHarris) */
    const char *cmap;        /* "viridis", "cube1_cmap", ... (same lookup; no hit -> cube1) */
    int32_t n;
    int32_t channel_mode, waterfall;
    double gain, range;
} sp_named_request;
int sp_render_named(sp_context *ctx, const sp_named_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply);
/* The same with a detector (enum sp_detector; sp_render_named is detector = SP_DETECTOR_SAMPLE).  The named request's layout is unchanged. */
int sp_render_named_ex(sp_context *ctx, const sp_named_request *req, int32_t detector, const uint8_t *bytes, size_t nbytes, int32_t width,
                       const sp_reply *reply);
/*
 * What the two option names of a named request resolve to (no device needed): the taper's plain name as sp_window takes it, the
 * colour map's key and its entry count (the caller sizes the reply's c_hist with it).  Any output may be NULL.
 */
int sp_named_resolve(const char *window, const char *cmap, const char **window_name, const char **cmap_key, int32_t *lut_len);
/*
 * How many plans - i.e. sets of taper / twiddle / LUT / threshold tables evaluated on the host and uploaded to the device - this
 * context has built so far, through sp_plan_create, sp_render or sp_render_named.  A request that repeats the previous one's
 * constants (sp_render: the same arrays by value; sp_render_named: the same names and numbers) does not add to it.
 */
int sp_context_plan_creations(const sp_context *ctx, int64_t *count);

/* Pre-evaluated request constants resident on the device: twiddles, taper, RGBA LUT, threshold tables. */
int sp_plan_create(sp_context *ctx, const sp_request *req, sp_plan **plan);
void sp_plan_destroy(sp_plan *plan);
/*
 * The frame loop on device-resident operands, asynchronous on the context's stream.
 * d_bytes: device pointer to the raw capture (nbytes bytes, 16-byte aligned); reply: device pointers.
 * Every output of the reply is overwritten, histograms included: a reply holds the counts of its own request, as the
 * reference's worker returns fresh arrays (lib/worker.js:40-41); the caller sums the slices (lib/spectroplot.js:1229-1238).
 * The reply's arrays must live in DEVICE memory of the context's device, c_hist / cb_hist / dbfs_minmax 8-byte aligned: the frame-loop
 * kernel clears them itself and its workgroups add their shares with device atomics (one kernel per call; no separate finish launch
 * for requests the frame loop covers).
 * Not capturable: every launch carries the number of its request, which its workgroups compare with what workgroup 0 publishes once it
 * has cleared the reply, so a launch replayed from a hipGraph would not wait.  A call on a stream that is being captured returns
 * SP_ERR_UNSUPPORTED.  (The wait relies on workgroup 0 being dispatched with the first wave of workgroups, as the hardware does; it is
 * bounded - a launch that never sees the number traps instead of hanging.  A trap is a failed launch: the HIP context of the PROCESS is
 * unusable afterwards - every later call returns SP_ERR_HIP - and can only be had back in a fresh process.)
 */
int sp_plan_execute(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const sp_reply *d_reply);
/*
 * The same request with the capture in HOST memory and the reply in DEVICE memory: the samples travel in chunks of frames on a copy
 * stream of the context while earlier chunks are rendered (the chunk schedule of sp_render; a sparse request uploads only the samples
 * its frames read), nothing comes back.  Returns once everything is queued: `bytes` must stay valid, and the reply is complete, when
 * the context's stream has been synchronised (page-locked `bytes`: the copies are asynchronous and at link rate).
 */
int sp_plan_execute_from_host(sp_plan *plan, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *d_reply);
/*
 * The caller's merge of slice replies (lib/spectroplot.js:1229-1238) on device-resident side outputs: `count` records of
 * [c_hist u64[lut_len] | cB_hist u64[SP_CB_HIST_SIZE] | dBfs_min f64 | dBfs_max f64] laid end to end at d_records (what an
 * all-gather of the slices' records delivers) are reduced to element-wise sums and min / max.  Outputs are device pointers;
 * any may be NULL.  Asynchronous on the context's stream.
 */
int sp_merge_replies(sp_context *ctx, const void *d_records, int32_t count, int32_t lut_len, uint64_t *d_c_hist, uint64_t *d_cb_hist,
                     double *d_dbfs_minmax);
/*
 * The same merge for a BATCH of renders in one launch: d_gathered holds what an all-gather of every rank's batch delivers -
 * [rank][render][record], `ranks` x `renders` records of lut_len + SP_CB_HIST_SIZE + 2 words - and d_merged receives `renders` merged
 * records [c_hist | cB_hist | dBfs_min, dBfs_max] end to end (device pointers).  What bench.py --gpus N runs once per collective
 * (one small launch per render between the frame loops costs a launch gap each).  Asynchronous on the context's stream.
 */
int sp_merge_replies_batch(sp_context *ctx, const void *d_gathered, int32_t ranks, int32_t renders, int32_t lut_len, void *d_merged);
/*
 * The caller's strip placement (lib/spectroplot.js:1241-1244: putImageData(strip, offset, 0), or (0, width - sliceWidth - offset) for the
 * waterfall layout) on device-resident strips: `count` strips of slice_width frames each, laid end to end at d_strips (what a gather of
 * the ranks' strips delivers, rank order), are placed in the merged image at d_image (n rows x width columns of RGBA, or width rows x n
 * columns for the waterfall layout).  Columns / rows beyond count * slice_width are left as they are (the caller's canvas keeps them
 * blank: clear the image first).  Asynchronous on the context's stream.
 */
int sp_place_strips(sp_context *ctx, uint8_t *d_image, const uint8_t *d_strips, int32_t count, int32_t n, int32_t width,
                    int32_t slice_width, int32_t waterfall);
/*
 * The caller's sliced render from one process (lib/spectroplot.js:1206-1244): a group owns one context per listed device (a device may be
 * listed more than once: every entry is a member with its own context and stream).  sp_group_render cuts the capture into
 * sp_group_size() slices as SampleView.slice does (lib/samples.js:253-258), uploads slice r to member r and renders it there - all
 * members at once - with sliceWidth = ~~(width / members) frames each; the strips and the slices' side outputs then travel to the root
 * member's device (member 0) without visiting host memory: grouped ncclSend / ncclRecv (RCCL over xGMI; librccl is loaded at run time)
 * when the members sit on distinct devices, peer copies otherwise or when SPECTROPLOT_HIP_NO_RCCL is set; there sp_merge_replies and
 * sp_place_strips do the caller's merge, and the merged image returns in ONE copy.
 * `reply` holds host pointers: rgba [4 * width * n] (columns beyond members * sliceWidth are zero, as the caller's canvas leaves them),
 * c_hist / cb_hist / dbfs_minmax merged over the slices (starting from 0 and (0, -200), :1125-1126), gauge_* [width] with slice r's
 * gauges at [r * sliceWidth, (r + 1) * sliceWidth).  Any may be NULL.  Plans are kept while the request's constants repeat.
 * sp_group_transport names what moved the strips in the last render: "none" (one member), "rccl", "peer" or "host".
 *
 * sp_group_render_ex chooses where the strips meet (sp_group_render = SP_GROUP_GATHER_DEVICE):
 *   SP_GROUP_GATHER_DEVICE  as above: the image is assembled in the root's HBM and comes back over the root's host link in one copy.
 *                           Peer copies and waterfall-layout RCCL receives land in the image itself (root memory = the image); the
 *                           spectrogram layout under RCCL receives whole strips next to it and re-tiles them on the root.  The mode
 *                           for an image that is consumed on the root GPU, and the one that exercises the xGMI gather.
 *   SP_GROUP_GATHER_HOST    the image is bound for the host anyway, so nothing is gathered on a device: every member runs the chunked
 *                           sp_render_strip pipeline on its own slice and copies its strip straight into its band of `reply->rgba`
 *                           over its OWN host link (N links side by side instead of one); histograms, dBfs range and gauges are
 *                           merged on the host.  transport = "host".  The mode to use whenever reply->rgba is host memory.
 * Environment (read when the group is created):
 *   SPECTROPLOT_HIP_NO_RCCL=1      never use RCCL
 *   SPECTROPLOT_HIP_FORCE_RCCL=1   use RCCL whatever the member list looks like: a one-member group then moves the root's own strip and
 *                                  record through a grouped self ncclSend / ncclRecv (what a one-GPU box can execute of the transport);
 *                                  members sharing a device make ncclCommInitAll fail, which falls back to peer copies like any other
 *                                  RCCL failure
 *   SPECTROPLOT_HIP_RCCL_LIB=path  the library to dlopen instead of librccl.so.1
 * An RCCL failure (library missing, init, send / receive, group end) never fails the render: the member streams are drained, the
 * communicators are aborted, the render is completed with peer copies, RCCL is not tried again on this group, and
 * sp_group_transport_note tells what happened (also: peer access that could not be enabled).
 * sp_group_last_timings: milliseconds of the last render's phases - upload + render (slowest member, device events), gather (from the
 * root's render to the assembled image on the root), download (root to host); in host mode the first is the slowest member's whole
 * sp_render_strip by the host clock and the other two are 0.
 */
typedef struct sp_group sp_group;
enum sp_group_gather { SP_GROUP_GATHER_DEVICE = 0, SP_GROUP_GATHER_HOST = 1 };
int sp_group_create(const int32_t *devices, int32_t count, sp_group **group);
void sp_group_destroy(sp_group *group);
int sp_group_size(const sp_group *group);
int sp_group_render(sp_group *group, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply);
int sp_group_render_ex(sp_group *group, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply,
                       int32_t gather);
const char *sp_group_transport(const sp_group *group);
const char *sp_group_transport_note(const sp_group *group);
int sp_group_last_timings(const sp_group *group, double *render_ms, double *gather_ms, double *download_ms);
/* Which RCCL this group has loaded: "<path of the library>, ncclGetVersion <code>, <n> communicator(s)"; empty while none is loaded. */
int sp_group_rccl_info(const sp_group *group, char *text, size_t capacity);
/* Device bytes the root member holds for the gather beyond its own strip (image + staging), after the last render. */
int sp_group_root_bytes(const sp_group *group, size_t *image_bytes, size_t *staging_bytes);
const char *sp_group_last_error(const sp_group *group);

/*
 * Batches: K captures rendered with ONE plan (format, n, taper, LUT, gain, range, channel mode and layout are the plan's).  Every item
 * gets, byte for byte, the reply sp_plan_execute / sp_render of that item alone gives (RGBA, gauges, both histograms, dBfs range): each
 * item is still one reference message (lib/worker.js:23-156).  Items have their own capture, byte length, width (so their own stride,
 * lib/worker.js:50) and reply buffers.  The frames of all items are dealt into groups of one size chosen from the batch's total frame
 * count, so small captures fill the chip (k_frames_batch, for 64 <= n <= 512; other plans render the items one by one, with the same
 * results).
 */
typedef struct sp_batch_item {
    const void *bytes;   /* the capture: host pointer (sp_render_batch) or device pointer, 16-byte aligned (sp_plan_execute_batch) */
    size_t nbytes;
    int32_t width;       /* frames of this item (0 and 1 allowed, with their single-request meaning) */
    int32_t reserved;
    sp_reply reply;      /* this item's outputs, host or device pointers as above; any may be NULL */
} sp_batch_item;
/*
 * Device-resident batch, asynchronous on the context's stream.  A small kernel clears every item's histograms and range first, then one
 * launch renders the items whose frames all lie inside their captures with the format's prefetching loader and one the others.  The
 * context's single-request state is not touched: single requests and batches may be interleaved on one context.  count == 0 queues
 * nothing; count < 0 or items == NULL with count > 0: SP_ERR_INVALID_ARG, as are misaligned reply arrays (see sp_plan_execute).  Not
 * capturable into a hipGraph (SP_ERR_UNSUPPORTED on a capturing stream).
 */
int sp_plan_execute_batch(sp_plan *plan, const sp_batch_item *items, int32_t count);
/*
 * The same on host buffers, synchronously: the captures are uploaded WHOLE (no sparse packing) into one device buffer at 16-byte aligned
 * offsets, the batch is rendered, each image comes back in one copy and the small outputs of all items in one.  A batch whose captures,
 * images and reply records need more than 256 MiB of device memory is rendered in sub-batches of at most that much (an item larger
 * than that alone).  Plans are cached as sp_render caches them; sp_context_last_upload_bytes reports the batch's upload total.
 */
int sp_render_batch(sp_context *ctx, const sp_request *req, const sp_batch_item *items, int32_t count);
/*
 * (tests) The work list sp_plan_execute_batch builds for a frame-loop plan with these shapes, without a device: out[] receives int64
 * words: frames per group, grid of the prefetching launch, grid of the generic launch, groups of each; then per item its launch
 * (0 prefetching, 1 generic loaders, 2 one by one through sp_plan_execute's path, 3 nothing to render: width 0, reply cleared only),
 * its first group in that launch and its group count.  *used = words needed (SP_ERR_INVALID_ARG if capacity is smaller).
 */
int sp_debug_batch_plan(int32_t format, int32_t n, int32_t lut_len, int32_t cu_count, const size_t *nbytes, const int32_t *widths,
                        int32_t count, int64_t *out, size_t capacity, size_t *used);

/*
 * (tests) The launch sp_plan_execute would make for a request of nbytes bytes and `width` frames on this plan's context, whose reply's
 * image is at `rgba` (only the address is looked at).  It is computed by the functions the launch path itself calls (request_shape,
 * request_kernel, frames_prefetch_width, frames_launch_rule, rgba_fast in sp_api.hip / sp_kernel_frames.h); nothing is launched.
 * out[] receives 11 int64 words: the kernel (0 nothing to render: width 0, 1 scratch_radix2, 3 k_frames, 4 k_frames_peak), log2 n,
 * channel mode, the prefetching loader's sample width (0: the generic loaders), frames per group, groups, workgroups, dynamic LDS
 * bytes (these four 0 behind the scratch kernel), whether the write-out stores the image in 16-byte pieces, the peak detector's
 * sub-frames per column (1: the sample detector's request), the context's CU count.  *used = words needed (SP_ERR_INVALID_ARG if
 * capacity is smaller).
 */
int sp_plan_debug_launch(const sp_plan *plan, size_t nbytes, int32_t width, const void *rgba, int64_t *out, size_t capacity, size_t *used);
/*
 * (tests) The launch rule of the three frame-loop kernels alone (frames_launch_rule, sp_kernel_frames.h), without a plan or a device:
 * `count` frames - or columns of a peak request - on a part with cu_count CUs (gf_fixed = 0), or `count` groups of gf_fixed frames
 * that a batch has dealt already.  out[] receives 4 int64 words: frames per group, groups, workgroups, dynamic LDS bytes.
 * SP_ERR_UNSUPPORTED where the rule refuses (n outside 64 ... 8192, lut_len outside 2 ... 256).
 */
int sp_debug_frames_launch(int32_t n, int32_t lut_len, int64_t count, int32_t cu_count, int32_t gf_fixed, int64_t *out, size_t capacity,
                           size_t *used);
/*
 * (tests) The launch shape of the portable ("scratch") kernels alone (scratch_blocks in sp_api.hip, scratch_wide in sp_launch.h), without
 * a plan or a device: one launch over `frames` frames - or columns of a peak request - at n = 2 ... SP_MAX_N on a part with cu_count
 * CUs, whose workgroups own `slabs` slabs of n doubles each (2: image and power plane, 3: a held peak, 4: traces).  out[] receives 2
 * int64 words: the workgroups - min(frames, 4 * cu_count, 256 MiB / (8 * slabs * n)), at least 1; workgroup b serves the frames
 * b, b + workgroups, ... - and whether the kernel is the variant that runs four radix-2 stages per barrier (n >= 4096).
 */
int sp_debug_scratch_launch(int32_t n, int32_t slabs, int32_t frames, int32_t cu_count, int64_t *out, size_t capacity, size_t *used);
/*
 * (tests) The CU count that shapes every launch on this context: the grids and frames per group of the six frame-loop kernels
 * (frames_launch_rule), a batch's work list, the scratch kernels' workgroups (at most 4 per CU), the pieces of a mean's accumulation
 * and the grid of sp_plan_power_to_db.  A context starts with its device's own count (hipGetDeviceProperties); cu_count = 1 ... that
 * count replaces it - an MI355X in a partition mode reports 128, 64 or 32 - and 0 puts the device's own back.  Anything else returns
 * SP_ERR_INVALID_ARG and changes nothing: no launch ever asks for more workgroups than the part at hand would be given without an
 * override.  Plans read the count when they launch, so the setting holds from the next call on the context, and
 * sp_plan_debug_launch reports it.  No reply depends on it, and the tests hold that.
 */
int sp_context_debug_set_cu_count(sp_context *ctx, int32_t cu_count);

/* Name of the kernel sp_plan_execute launches: "frames" (64 <= n <= 8192, LUT <= 256 entries) or "scratch_radix2" (everything else).
 * A peak plan answers what its M >= 2 requests take: "frames_peak" (64 <= n <= 1024 and what "frames" asks for) or "scratch_radix2". */
const char *sp_plan_kernel_name(const sp_plan *plan);
/*
 * The same for a request of this shape: a peak plan answers "frames_peak" where k_frames_peak renders it (M >= 2, 64 <= n <= 1024 and
 * everything "frames" asks for), "scratch_radix2" for its other M >= 2 requests (the portable kernel holds the peak too), and what
 * sp_plan_kernel_name answers when M == 1.  A sample plan answers sp_plan_kernel_name's.
 */
const char *sp_plan_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);
/* Forces a kernel (tests compare the two device paths): 0 automatic, 1 scratch_radix2, 3 frames (2: removed, SP_ERR_UNSUPPORTED).
 * On a peak plan 3 means frames for M == 1 requests and frames_peak for M >= 2 requests where it covers the plan's n (64 ... 1024);
 * the plan's other M >= 2 requests take scratch_radix2 (sp_plan_kernel_name_for tells). */
int sp_plan_force_kernel(sp_plan *plan, int32_t which);

/*
 * Per-bin min / max traces over a request: what a spectrum viewer draws as its min-hold and max-hold traces.
 * The request's frames are sp_plan_execute's (the same geometry, limits and statuses; channel mode honoured).  With
 * d(x, i) = dBfs - gain of frame x, bin i exactly as lib/worker.js:92-93, 102 computes it, the fold runs in order of x:
 *     trace_min[y] = 0.0;   if (d(x, i) < trace_min[y]) trace_min[y] = d(x, i)
 *     trace_max[y] = -200;  if (d(x, i) > trace_max[y]) trace_max[y] = d(x, i)
 * with y = i <= n/2 ? n/2 - i : n/2 + n - i (worker.js:90): trace_*[y] belongs to image row y of the spectrogram layout and to
 * column n - 1 - y of the waterfall layout, and the arrays are the same for both layouts.  This is the worker's own fold of a
 * column's extremes (gauge_mins / gauge_maxs) with its own start values, turned by 90 degrees: a NaN never wins; a bin that is NaN
 * in every column, and width == 0, give (0, -200); an all-zero frame gives trace_min = -inf.  Hence, bit for bit,
 * min over y of trace_min[y] == dBfs_min and max over y of trace_max[y] == dBfs_max of sp_render on the same request.
 * The outputs are two f64[n] arrays; either may be NULL.  No image is written and no other reply field is produced.
 * Only plans of the sample detector are accepted: a peak plan returns SP_ERR_UNSUPPORTED.  (The mean-power trace is sp_plan_execute_mean
 * below: an f64 sum over frames would depend on the deal of frames to workgroups, so it is an exact sum; min and max need none.)
 *
 * sp_plan_execute_traces: device-resident operands, asynchronous on the context's stream; d_trace_min / d_trace_max are device
 * pointers, 8-byte aligned (SP_ERR_INVALID_ARG otherwise).  Three kernels and no request number: a stream that is being captured is
 * not refused.
 * sp_render_traces: host buffers, synchronous, the plan cached as by sp_render.  The samples travel as for a request whose image
 * stays on the device (sp_plan_execute_from_host): a sparse request (stride > n) uploads only what its frames read, a large one
 * travels in chunks of frames under the frame loops of earlier chunks; sp_context_last_upload_bytes reports what travelled.
 * sp_plan_traces_kernel_name_for: "frames_traces" (64 <= n <= 1024 and a finite taper; LUT length and edge ranges do not matter)
 * or "scratch_traces" (everything else).  sp_plan_force_kernel applies as to renders: 1 forces "scratch_traces", 3 means
 * "frames_traces" where that kernel covers the plan.
 */
int sp_plan_execute_traces(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_trace_min, double *d_trace_max);
int sp_render_traces(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, double *trace_min,
                     double *trace_max);
const char *sp_plan_traces_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);

/*
 * Power plane replies: the numeric spectrogram behind every other reply, |X|^2 per frame and bin as f64.
 * `power` is double[width * n], frame-major:
 *     power[x * n + y] = real[i] * real[i] + imag[i] * imag[i]
 * of frame x, bin i exactly as lib/worker.js:70-92 computes it - behind the taper, the transform and, in channel mode, splitreal; two
 * multiplies and one add, never contracted - with y = i <= n/2 ? n/2 - i : n/2 + n - i (worker.js:90): y is image row y of the
 * spectrogram layout and column n - 1 - y of the waterfall layout, as for the traces and the density, and the plan's `waterfall` flag
 * does not change the array.  The request's frames are sp_plan_execute's (the same geometry, positions, limits and statuses; channel
 * mode honoured).  A frame that reads past the capture gives NaN, as the reference does, and A NaN IS ANY NaN: its payload and sign
 * are unspecified.  Every other value is bit-exact, +0.0, +inf and denormals included; |X|^2 is never -0.  width == 0 writes nothing
 * and returns SP_OK.  Gain, range, LUT and block_norm do not reach the plane.  A plane has no reduction, so it does not depend on the
 * deal of frames to workgroups (the CU count).
 * Only plans of the sample detector are accepted: a peak plan returns SP_ERR_UNSUPPORTED, as for the traces.
 * The dB plane is db[k] = (5 * log10(power[k]) + block_norm_db + gain) - gain in exactly that operation order (worker.js:93, 100),
 * log10 the engine's function as the library restates it: 0 gives -inf, NaN gives NaN.
 *
 * sp_plan_execute_power: device operands, asynchronous on the context's stream.  d_power must be 8-byte aligned and non-NULL when
 *   width > 0 (SP_ERR_INVALID_ARG otherwise).  ONE launch, no workspace of the context's beyond the portable kernel's slabs, no request
 *   number, handshake, bounded wait or trap: a stream that is being captured is not refused, and the call may be interleaved with
 *   sp_plan_execute / _index / _traces on one context without a synchronisation.  All plane offsets are 64-bit (8 * width * n may pass
 *   4 GiB).
 * sp_plan_power_to_db: d_db[k] = db of d_power[k] for k < count with the plan's block_norm_db and gain, asynchronous on the context's
 *   stream; both pointers 8-byte aligned device pointers (SP_ERR_INVALID_ARG otherwise); d_db == d_power converts in place;
 *   count == 0 queues nothing.
 * sp_render_power: host buffers, synchronous, the plan cached as by sp_render.  The capture travels as for sp_render - a packed upload
 *   where stride > n, chunks of frames where the request is large (the plane, 8 * width * n bytes, counts as the reply that comes
 *   back) - and rows [x0, x1) of the plane come back behind every chunk in one contiguous copy; with db != 0 they are converted in
 *   place on the device first, so `power` then holds the dB plane.  `power` must be 8-byte aligned and non-NULL when width > 0.
 *   sp_context_last_upload_bytes / sp_context_last_chunks report as before.
 * sp_plan_power_kernel_name_for: "frames_power" - k_frames_power, k_frames' frame loop with one 8-byte store per bin - where
 *   "frames_traces" would be answered (64 <= n <= 1024, a finite taper, the plan not forced to kernel 1), or "scratch_power" for
 *   everything else.  sp_plan_force_kernel applies as to the traces.
 * Out of scope: the held plane of a peak plan, batches, groups, sharding.py, and a [y][x] (spectrogram-major) plane.
 */
int sp_plan_execute_power(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_power);
int sp_plan_power_to_db(sp_plan *plan, const double *d_power, size_t count, double *d_db);
int sp_render_power(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t db, double *power);
const char *sp_plan_power_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);

/*
 * Exact mean-power trace: the average spectrum of a request (a Welch PSD), bit-exact like the min and max traces.
 * With power[x][y] the value sp_plan_execute_power writes for frame x and image row y - the same geometry, limits, statuses, channel
 * mode and row order y = i <= n/2 ? n/2 - i : n/2 + n - i (worker.js:90) - `mean` is double[n]:
 *     mean[y] = RN( sum over x in [0, width) of power[x][y] ) / (double)width
 * The sum is the EXACT real-number sum.  RN is one IEEE-754 round-to-nearest-even to f64; a sum at or above 2^1024 - 2^970 gives +inf.
 * The division is one correctly rounded f64 division.  In Python: math.fsum(column) / width, with OverflowError read as +inf.
 * A row with a NaN in any frame is NaN, and A NaN IS ANY NaN, as for the plane; otherwise a row with +inf in any frame is +inf.
 * width == 0 writes NaN to all n entries (0 / 0).  The array is the same for both layouts and does not depend on gain, range, LUT or
 * block_norm.  Only plans of the sample detector are accepted: a peak plan returns SP_ERR_UNSUPPORTED, as for the plane and the
 * traces.  The dB form is sp_plan_power_to_db applied to the n means: the dB of the mean power, NOT the mean of the dB values.
 * How: |X|^2 is never negative, so every value is a 53-bit integer times a power of two; the values are added into a wide fixed-point
 * accumulator per row (66 64-bit cells, cell k weighing 2^(32 k - 1074), and a count of NaNs and of +inf) with integer adds only, and
 * the accumulator is rounded once.  Integer adds commute: THE RESULT DOES NOT DEPEND ON THE CU COUNT, THE DEAL OF FRAMES TO WORKGROUPS,
 * THE CHUNKING OF A HOST-FED REQUEST OR THE WINDOW DESCRIBED BELOW.
 * Cost: a workspace of the context, (66 + 2) * 8 * n bytes of device memory (0.5 MiB at n = 1024, 544 MiB at SP_MAX_N), grown and
 * never shrunk, cleared on the stream by every request.
 *
 * sp_power_mean: the mean of a frame-major plane double[width * n] the caller holds on the device; the companion of
 *   sp_plan_power_to_db, as sp_density_from_index is of the index image.  Asynchronous on the context's stream; it carries no request
 *   number, so a stream that is being captured is not refused.  n >= 1 (any n, not only powers of two), width >= 0, both pointers
 *   8-byte aligned, d_mean non-NULL, d_power non-NULL when width > 0 (SP_ERR_INVALID_ARG otherwise).  The values must not be negative:
 *   the sign bit of a value is not looked at.
 * sp_plan_execute_mean: device operands, asynchronous.  The plane is never held whole: the frames are rendered block by block by
 *   sp_plan_execute_power's frame loop (k_frames_power or k_scratch_power; sp_plan_force_kernel applies) into a bounded window of the
 *   context - 64 MiB by default and at least one frame - and accumulated behind each block; then the sum is finished.  The checks are
 *   sp_plan_execute_power's; d_mean must be 8-byte aligned and non-NULL (SP_ERR_INVALID_ARG otherwise).  No request number: the call
 *   may be interleaved with sp_plan_execute / _index / _power on one context without a synchronisation.
 * sp_render_mean: host buffers, synchronous, the plan cached as by sp_render.  The samples are the only bulk transfer and travel as for
 *   sp_render_traces - a packed upload where stride > n, chunks of frames where the request is large; every chunk's frames are rendered
 *   into the window and accumulated behind its upload, and n doubles come back in one copy, converted to dB on the device first when
 *   db != 0.  `mean` must be 8-byte aligned and non-NULL.  sp_context_last_upload_bytes / sp_context_last_chunks report as before.
 * sp_context_set_mean_window: (tests) the window's size in bytes; 0 restores the default.  A window below one frame holds one frame.
 * sp_debug_exact_sum: (tests, no device needed) *sum = RN(exact sum) of `count` non-negative values through the host side of the code
 *   the kernels run, with the NaN and inf rule; the empty sum is +0.0.  A negative value, -0.0 or -inf returns SP_ERR_INVALID_ARG.
 * sp_plan_mean_kernel_name_for: "frames_power+mean" or "scratch_power+mean", following sp_plan_power_kernel_name_for.
 * Out of scope: peak plans, batches, groups and sharding.py (their merge would be an element-wise integer sum of the cells),
 * accumulation over successive captures, the accumulation fused into the frame loop, and a bound on the workspace.
 */
int sp_power_mean(sp_context *ctx, const double *d_power, int32_t n, int32_t width, double *d_mean);
int sp_plan_execute_mean(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_mean);
int sp_render_mean(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t db, double *mean);
int sp_context_set_mean_window(sp_context *ctx, size_t bytes);
/* (tests, no device needed) The grid of the accumulation behind `frames` >= 1 frames of a plane of n rows on a part with cu_count CUs:
 * out[] receives 3 int64 words - the bands of 64 rows, the pieces the frames are cut into (about 4 workgroups per CU, no piece below 32
 * frames) and the frames per piece (the last piece may be shorter).  *used = words needed (SP_ERR_INVALID_ARG if capacity is smaller). */
int sp_debug_mean_launch(int32_t n, int64_t frames, int32_t cu_count, int64_t *out, size_t capacity, size_t *used);
int sp_debug_exact_sum(const double *values, size_t count, double *sum);
const char *sp_plan_mean_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);

/*
 * Exact variance and spectral-kurtosis traces: the second-order statistics of every image row over the request's frames - the confidence
 * band of the Welch PSD the mean trace gives, and the spectral-kurtosis detector SK = (W + 1) / (W - 1) * (W * S2 / S1^2 - 1), about 1
 * for Gaussian noise, below 1 for a steady carrier, above 1 for bursts.  Bit-exact like the mean trace.
 * With power[x][y] the value sp_plan_execute_power writes for frame x and image row y (`abs2` of lib/worker.js:70-92 in the image row
 * order of worker.js:90; the reference has no such fold) - the geometry, limits, statuses, channel mode and row order of
 * sp_plan_execute_mean - and W = width, the reply is double[3 * n], three arrays of n:
 *     out[0 * n + y] = RN( S1 ),              S1 = sum over x in [0, W) of power[x][y]         out[0][y] / W is sp_*_mean's value, bit for bit
 *     out[1 * n + y] = RN( S2 ),              S2 = sum over x in [0, W) of power[x][y]^2
 *     out[2 * n + y] = RN( W * S2 - S1^2 )    W^2 times the population variance of the row
 * Every sum, square, product and the difference is the EXACT real number - a square is a 106-bit product, nothing is rounded before
 * the one RN - so out[2] never suffers the cancellation of W * S2 - S1^2: a row that is constant over the frames gives +0.0 exactly, a
 * row that differs by one ulp in one frame gives the exact tiny positive value, and no result is ever negative (Cauchy-Schwarz).  RN is
 * one IEEE-754 round-to-nearest-even to f64, INTO THE DENORMAL RANGE where the exact value lies there (a square goes down to 2^-2148),
 * and +inf where it rounds past DBL_MAX: out[1] or out[2] may be +inf where out[0] is finite.  In Python, per row:
 * float(sum(Fraction(v))), float(sum(Fraction(v) ** 2)), float(W * sum(Fraction(v) ** 2) - sum(Fraction(v)) ** 2), OverflowError read
 * as +inf.
 * SPECIAL VALUES follow the mean's rule and apply to all three arrays of the row: a NaN in any frame gives NaN (A NaN IS ANY NaN);
 * otherwise +inf in any frame gives +inf.  width == 0 writes 3 * n times +0.0, the sums of nothing.  The arrays do not depend on gain,
 * range, LUT or block_norm, NOR ON THE CU COUNT, THE DEAL OF FRAMES TO WORKGROUPS, THE WINDOW OR THE CHUNKING OF A HOST-FED REQUEST
 * (integer adds commute).  Only plans of the sample detector are accepted: a peak plan returns SP_ERR_UNSUPPORTED.
 * The derived quantities stay with the caller, and neither form contains a cancellation:
 *     population variance out[2] / (W * W), sample variance out[2] / (W * (W - 1));     SK = (W + 1) / (W - 1) * out[2] / out[0]^2
 * How: csrc/sp_variance_core.h.  Every value is read once; its three 32-bit pieces go to the 66 cells of S1 as for the mean, and its
 * square m^2 << 2 (e - 1), in units of 2^-2148, is cut into five pieces for 132 cells of S2; integer adds only.  The finish forms
 * W * S2 and S1^2 digit by digit, subtracts with a borrow and rounds the digit string once.
 * Cost: a workspace of the context of its own, (66 + 132 + 2) * 8 * n bytes (1.6 MiB at n = 1024, 1.6 GiB at SP_MAX_N), grown and
 * never shrunk, cleared on the stream by every request.
 *
 * sp_power_variance: over a frame-major plane double[width * n] the caller holds on the device; the companion of sp_power_mean.
 *   Asynchronous on the context's stream, no request number.  1 <= n <= SP_MAX_N (any n), width >= 0, both pointers 8-byte aligned,
 *   d_out non-NULL, d_power non-NULL when width > 0 (SP_ERR_INVALID_ARG otherwise, and nothing is written).  The values must not be
 *   negative: the sign bit of a value is not looked at.
 * sp_plan_execute_variance: device operands, asynchronous.  The plane passes block by block through the mean's window
 *   (sp_context_set_mean_window applies) and is accumulated behind each block; then the rows are finished.  The checks are
 *   sp_plan_execute_power's, then the output's.  No request number: the call may be interleaved with sp_plan_execute / _power / _mean
 *   on one context without a synchronisation.
 * sp_render_variance: host buffers, synchronous, the plan cached as by sp_render.  The samples travel as for sp_render_mean and 3 * n
 *   doubles come back in one copy.  There is no db argument: a sum of squares has no dB form.
 * sp_debug_variance_sums: (tests, no device needed) out3[0 .. 2] of one row of `count` < 2^31 non-negative values (W = count) through
 *   the host side of the code the kernels run, with the NaN and inf rule; no values give three times +0.0.  A negative value, -0.0
 *   or -inf returns SP_ERR_INVALID_ARG and writes nothing.
 * sp_debug_variance_launch: (tests, no device needed) the grid of the accumulation behind `frames` >= 1 frames of a plane of n rows on
 *   a part with cu_count CUs: out[] receives 3 int64 words - the bands of 32 rows, the pieces the frames are cut into (about 6
 *   workgroups per CU, no piece below 32 frames) and the frames per piece (the last piece may be shorter).  *used = words needed
 *   (SP_ERR_INVALID_ARG if capacity is smaller).
 * sp_plan_variance_kernel_name_for: "frames_power+variance" or "scratch_power+variance", following sp_plan_power_kernel_name_for.
 * Out of scope: the Node addon (its export table is pinned), peak plans, batches, groups and sharding.py, covariances between rows,
 * higher moments (skewness), and the accumulation fused into the frame loop.
 */
int sp_power_variance(sp_context *ctx, const double *d_power, int32_t n, int32_t width, double *d_out);
int sp_plan_execute_variance(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, double *d_out);
int sp_render_variance(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, double *out);
int sp_debug_variance_sums(const double *values, size_t count, double *out3);
int sp_debug_variance_launch(int32_t n, int64_t frames, int32_t cu_count, int64_t *out, size_t capacity, size_t *used);
const char *sp_plan_variance_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);

/*
 * Exact band-power series: the power of a band of image rows per frame - the zero-span / channel-power trace of a spectrum analyser,
 * the envelope of one transmitter in a crowded capture - bit-exact like the mean.  The mean is the plane's marginal along x, this is
 * its marginal along y.
 * With power[x][y] the value sp_plan_execute_power writes for frame x and image row y - the same geometry, limits, statuses, channel
 * mode and row order y = i <= n/2 ? n/2 - i : n/2 + n - i (worker.js:90) - a band is a half-open range of image rows [y0, y1) with
 * 0 <= y0 <= y1 <= n.  The bands are a HOST array int32_t bands[2 * count] = {y0_0, y1_0, y0_1, y1_1, ...}, read before the call
 * returns; 0 <= count <= SP_MAX_BANDS; bands may overlap and may be empty.  The reply is double[count * width], BAND-MAJOR, so every
 * band is one contiguous time series:
 *     band[b * width + x] = RN( sum over y in [y0_b, y1_b) of power[x][y] )
 * The sum is the EXACT real-number sum and RN is one IEEE-754 round-to-nearest-even to f64, as for the mean; a sum at or above
 * 2^1024 - 2^970 gives +inf.  A band with a NaN addend is NaN, and A NaN IS ANY NaN; otherwise a band with a +inf addend is +inf.  An
 * empty band gives +0.0.  The value is a SUM, not a mean: the power of a channel is the sum of its bins.  In Python:
 * math.fsum(plane[x, y0:y1]) with OverflowError read as +inf; a band of one row therefore equals the plane's column bit for bit.
 * width == 0 or count == 0 writes nothing and returns SP_OK.  The array is the same for both layouts and does not depend on gain,
 * range, LUT or block_norm, NOR ON THE CU COUNT, THE WINDOW OR THE CHUNKING OF A HOST-FED REQUEST (integer adds commute).  Only plans of
 * the sample detector are accepted: a peak plan returns SP_ERR_UNSUPPORTED, as for the plane and the mean.  The dB form is
 * sp_plan_power_to_db applied to the count * width sums.
 * SP_ERR_INVALID_ARG: a band outside 0 <= y0 <= y1 <= n, count outside 0 .. SP_MAX_BANDS, bands == NULL with count > 0, a NULL or
 * misaligned (8 bytes) output when count * width > 0.
 * How: the mean's accumulator (66 64-bit cells and two counters, integer adds only, rounded once) per FRAME instead of per row.  A
 * frame's rows are summed inside one workgroup, in LDS, and finished there: no workspace of the context, no clear and no finishing
 * launch.
 *
 * sp_band_rows: (pure host arithmetic, no device needed) the rows whose centre frequency lies in [f_lo, f_hi], in cycles per sample:
 *   row y is centred on f(y) = (n/2 - y) / n, so row 0 is +1/2, row n/2 is DC and row n - 1 is -1/2 + 1/n.
 *     *y0 = clamp(ceil(n/2 - f_hi * n), 0, n)        *y1 = clamp(floor(n/2 - f_lo * n) + 1, 0, n), raised to *y0 if below it
 *   computed in f64 in exactly that order.  SP_ERR_INVALID_ARG for a NaN, for f_lo > f_hi, for n < 2 and for a NULL output;
 *   SP_ERR_NOT_POW2 as elsewhere.  In channel mode the rows are the L/R split's (L above R), not one frequency axis: the helper is
 *   for I/Q plans.
 * sp_power_bands: the sums over a frame-major plane double[width * n] the caller holds on the device; the companion of sp_power_mean.
 *   Asynchronous on the context's stream, ONE launch, no workspace of the context and no request number: a stream that is being
 *   captured is not refused.  n >= 1 (any n, not only powers of two), width >= 0; d_power (non-NULL when count * width > 0) and d_band
 *   8-byte aligned device pointers.  The values must not be negative: the sign bit of a value is not looked at.
 * sp_plan_execute_bandpower: device operands, asynchronous.  The plane is never held whole: it passes block by block through the
 *   mean's window (sp_context_set_mean_window applies) and the sums of the block's frames, columns [x0, x1) of every band, are made
 *   behind each block.  The checks are sp_plan_execute_power's, then the bands'.  No request number: the call may be interleaved with
 *   sp_plan_execute / _index / _power / _mean on one context without a synchronisation.
 * sp_render_bandpower: host buffers, synchronous, the plan cached as by sp_render.  The samples are the only bulk transfer and travel
 *   as for sp_render_mean - a packed upload where stride > n, chunks of frames where the request is large - and count * width doubles
 *   come back in one copy, converted to dB on the device first when db != 0.  sp_context_last_upload_bytes / sp_context_last_chunks
 *   report as before.
 * sp_plan_bandpower_kernel_name_for: "frames_power+bands" or "scratch_power+bands", following sp_plan_power_kernel_name_for.
 * Out of scope: peak plans, batches, groups and sharding.py (a shard's frames are a run of columns of every band), the sum fused into
 * the frame loop, and weighted bands.
 */
#define SP_MAX_BANDS 64
int sp_band_rows(int32_t n, double f_lo, double f_hi, int32_t *y0, int32_t *y1);
int sp_power_bands(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, double *d_band);
int sp_plan_execute_bandpower(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                              double *d_band);
int sp_render_bandpower(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                        int32_t count, int32_t db, double *band);
const char *sp_plan_bandpower_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);

/*
 * Exact spectral moments: where a band's power lies and how wide it is, per frame - the power-weighted sums from which the caller takes
 * the centroid (the discriminator output of an FSK capture, a sub-bin frequency estimate that the peak track's argmax cannot give) and
 * the RMS bandwidth of a burst (without the threshold the occupancy counts need).  Bit-exact like the band-power series.
 * With power[x][y], the bands (a HOST array of `count` pairs [y0, y1), 0 <= count <= SP_MAX_BANDS, read before the call returns, bands
 * may overlap and may be empty), the geometry, limits, statuses, channel mode and row order of sp_plan_execute_bandpower, and `order` 0,
 * 1 or 2, the reply is double[(order + 1) * count * width], MOMENT-MAJOR, then band-major, so each moment of each band is one contiguous
 * time series:
 *     m[(k * count + b) * width + x] = RN( sum over y in [y0_b, y1_b) of (y - y0_b)^k * power[x][y] ),   k = 0 .. order,   0^0 = 1
 * The weights count rows from the band's FIRST row, so they are small integers below 2^20 (squared: below 2^40).  The sum is the EXACT
 * real-number sum and RN is one IEEE-754 round-to-nearest-even to f64; a sum at or above 2^1024 - 2^970 gives +inf.  m[0] is the
 * band-power series bit for bit.  In Python: float(sum(Fraction(y - y0) ** k * Fraction(v))) with OverflowError read as +inf.
 * SPECIAL VALUES ARE THE BAND'S, NOT THE TERM'S: if any row of the band in that frame is a NaN, every moment of that (band, frame) is
 * NaN (A NaN IS ANY NaN); otherwise, if any row is +inf, every moment is +inf - also where the row's weight is 0, where an IEEE 0 * inf
 * would be a NaN: a band that holds a special value has no centroid, and says so in every series.  An empty band gives +0.0 in every
 * moment; a band of one row gives m[1] = m[2] = +0.0.  width == 0 or count == 0 writes nothing and returns SP_OK.  The arrays are the
 * same for both layouts and do not depend on gain, range, LUT or block_norm, NOR ON THE CU COUNT, THE WINDOW OR THE CHUNKING OF A
 * HOST-FED REQUEST (integer adds commute).  Only plans of the sample detector are accepted: a peak plan returns SP_ERR_UNSUPPORTED, as
 * for the band-power series.
 * The derived quantities stay with the caller, one or two IEEE operations each on the reply:
 *     centroid row y0 + m1 / m0;   centroid frequency (n/2 - y0 - m1 / m0) / n cycles per sample (I/Q plans);
 *     RMS width in rows sqrt(m2 / m0 - (m1 / m0)^2) - which cancels on a wide band: measure a width with a tight band.
 * SP_ERR_INVALID_ARG: an order outside 0 .. 2, a band outside 0 <= y0 <= y1 <= n, count outside 0 .. SP_MAX_BANDS, bands == NULL with
 * count > 0, n > SP_MAX_N, a NULL or misaligned (8 bytes) output when count * width > 0 - all before the device is touched.
 * How: the band-power kernel's shape with one accumulator of 68 64-bit cells per moment in LDS (csrc/sp_moment_core.h: the value's
 * 53-bit integer times its weight, cut into four 32-bit pieces) and the NaN and +inf counters shared; integer adds only, rounded once,
 * no workspace of the context, no clear and no finishing launch.  The kernel is compiled per order: order 1 does not pay for m2.
 *
 * sp_power_moments: the moments over a frame-major plane double[width * n] the caller holds on the device; the companion of
 *   sp_power_bands.  Asynchronous on the context's stream, ONE launch, no workspace and no request number.  1 <= n <= SP_MAX_N (any n),
 *   width >= 0; d_power (non-NULL when count * width > 0) and d_out 8-byte aligned device pointers.  The values must not be negative.
 * sp_plan_execute_moments: device operands, asynchronous.  The plane passes block by block through the mean's window
 *   (sp_context_set_mean_window applies) and the block's columns [x0, x1) of every series are made behind each block.  The checks are
 *   sp_plan_execute_power's, then the order's, the bands' and the output's.  No request number: the call may be interleaved with
 *   sp_plan_execute / _power / _mean / _bandpower on one context without a synchronisation.
 * sp_render_moments: host buffers, synchronous, the plan cached as by sp_render.  The samples travel as for sp_render_bandpower and
 *   (order + 1) * count * width doubles come back in one copy.  db != 0 converts m[0] ONLY, the first count * width values, as
 *   sp_plan_power_to_db does; m[1] and m[2] have no dB form and come back as they are.
 * sp_debug_moment_sum: (tests, no device needed) out[k] = RN(exact sum of r^k * values[r]), k = 0 .. order, of one column of `count` <=
 *   SP_MAX_N non-negative values with the weights r = 0 .. count - 1, through the host side of the code the kernel runs, with the NaN
 *   and inf rule; out holds order + 1 doubles.  A negative value, -0.0 or -inf, a bad order or a longer column returns
 *   SP_ERR_INVALID_ARG and writes nothing.
 * sp_plan_moments_kernel_name_for: "frames_power+moments" or "scratch_power+moments", following sp_plan_power_kernel_name_for.
 * Out of scope: the Node addon (its export table is pinned), peak plans, batches, groups and sharding.py, per-burst centroids,
 * arbitrary f64 weights, and the sums fused into the frame loop.
 */
int sp_power_moments(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, int32_t order,
                     double *d_out);
int sp_plan_execute_moments(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                            int32_t order, double *d_out);
int sp_render_moments(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                      int32_t count, int32_t order, int32_t db, double *out);
int sp_debug_moment_sum(const double *values, size_t count, int32_t order, double *out);
const char *sp_plan_moments_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);

/*
 * Peak track: the strongest row of a band of image rows, and its power, per frame - the peak search of a spectrum analyser per sweep,
 * over time the frequency-versus-time track of a transmitter (the two tones of an FSK burst, a drifting carrier, a chirp); the
 * companion of the band-power series, which shows the same burst's amplitude.  gauge_maxs is no substitute: one clamped byte for the
 * whole spectrum, which names no row and cannot be restricted to a band.
 * With power[x][y] the value sp_plan_execute_power writes for frame x and image row y (abs2 of lib/worker.js:85-92) - the same
 * geometry, limits, statuses, channel mode and row order y = i <= n/2 ? n/2 - i : n/2 + n - i (worker.js:90) - the bands are exactly the
 * band-power series' bands: a HOST array int32_t bands[2 * count] of half-open row ranges [y0, y1) with 0 <= y0 <= y1 <= n, read before
 * the call returns; 0 <= count <= SP_MAX_BANDS; bands may overlap and may be empty.  The reply is two BAND-MAJOR arrays, so every band
 * is one contiguous time series: int32_t row[count * width] and double peak[count * width].  For band b and frame x, over the rows y in
 * [y0_b, y1_b) whose power[x][y] is not a NaN:
 *     peak[b * width + x] = the largest such value, bit for bit as the plane holds it (+inf can win; an all-zero frame gives +0.0)
 *     row[b * width + x]  = the row that holds it; among equal values THE SMALLEST y WINS
 * and for an empty band, or a band whose rows are all NaN in that frame, row = -1 and peak = NaN.  A NaN IS ANY NaN, as everywhere
 * else; a capture shorter than n therefore gives -1 / NaN throughout.  In numpy, per frame: p = plane[x, y0:y1]; (-1, nan) if p is
 * empty or all NaN, else k = argmax(where(isnan(p), -1.0, p)) and (y0 + k, p[k]).  A band of one row gives that row's index and the
 * plane's column bit for bit wherever the column is not NaN.
 * width == 0 or count == 0 writes nothing and returns SP_OK.  Either output may be NULL and is not written then; both NULL with
 * count * width > 0 is SP_ERR_INVALID_ARG, and so is a `row` that is not 4-byte aligned or a `peak` that is not 8-byte aligned, a band
 * outside 0 <= y0 <= y1 <= n, count outside 0 .. SP_MAX_BANDS and bands == NULL with count > 0.  The arrays are the same for both
 * layouts and do not depend on gain, range, LUT or block_norm, NOR ON THE CU COUNT, THE WINDOW OR THE CHUNKING OF A HOST-FED REQUEST (a
 * maximum with a fixed tie rule commutes).  Only plans of the sample detector are accepted: a peak plan returns SP_ERR_UNSUPPORTED, as
 * for the plane, the mean and the bands.  The dB form is sp_plan_power_to_db applied to `peak`; NaN stays NaN.
 * How: no floating-point compare anywhere.  The KEY of a value is its bit pattern with the sign bit cleared; non-negative doubles and
 * +inf order as their keys do as unsigned integers, and a key above 0x7ff0000000000000 is a NaN.  The larger key wins and on an equal
 * key the smaller row (csrc/sp_track_core.h, the one place the decision is made, for the kernel and for sp_debug_band_peak).  One
 * launch behind every block of frames: no workspace of the context, no clear, no atomics, no second launch.
 *
 * sp_power_tracks: the track over a frame-major plane double[width * n] the caller holds on the device; the companion of
 *   sp_power_bands.  Asynchronous on the context's stream, ONE launch, no workspace of the context and no request number: a stream
 *   that is being captured is not refused.  n >= 1 (any n, not only powers of two), width >= 0; d_power (non-NULL when
 *   count * width > 0) an 8-byte aligned device pointer.  The values must not be negative: the sign bit of a value is not looked at,
 *   and a NaN of either sign is a NaN; what comes back for a value whose sign bit is set is unspecified beyond that.
 * sp_plan_execute_track: device operands, asynchronous.  The plane is never held whole: it passes block by block through the mean's
 *   window (sp_context_set_mean_window applies) and the track of the block's frames, columns [x0, x1) of every band, is made behind
 *   each block.  The checks are sp_plan_execute_power's, then the bands', then the outputs'.  No request number: the call may be
 *   interleaved with sp_plan_execute / _power / _mean / _bandpower on one context without a synchronisation.
 * sp_render_track: host buffers, synchronous, the plan cached as by sp_render.  The samples are the only bulk transfer and travel as
 *   for sp_render_bandpower - a packed upload where stride > n, chunks of frames where the request is large - and `row` and `peak`
 *   come back in one copy each, `peak` converted to dB on the device first when db != 0.  sp_context_last_upload_bytes /
 *   sp_context_last_chunks report as before.
 * sp_plan_track_kernel_name_for: "frames_power+track" or "scratch_power+track", following sp_plan_power_kernel_name_for.
 * sp_debug_band_peak: (tests, no device needed) *row and *peak of the rows [y0, y1) of one frame's `n` values through the host side of
 *   the code the kernel runs.  SP_ERR_INVALID_ARG for values == NULL, n < 1, a band outside 0 <= y0 <= y1 <= n, or both outputs NULL
 *   (either one may be).
 * Out of scope: peak plans, batches, groups and sharding.py (a shard's frames are a run of columns of every band, and their merge is
 * trivial), the search fused into the frame loop, more than one peak per band, sub-bin interpolation, and a threshold.
 */
int sp_power_tracks(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count,
                    int32_t *d_row, double *d_peak);
int sp_plan_execute_track(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                          int32_t *d_row, double *d_peak);
int sp_render_track(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                    int32_t count, int32_t db, int32_t *row, double *peak);
const char *sp_plan_track_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);
int sp_debug_band_peak(const double *values, int32_t n, int32_t y0, int32_t y1, int32_t *row, double *peak);

/*
 * Occupancy counts: how often a row reaches a threshold, and how many rows of a band reach theirs in a frame - per row the duty cycle
 * or channel occupancy of a monitoring receiver (rows[y] / width), per frame and band the occupied-bandwidth trace of a burst.
 * With power[x][y] the value sp_plan_execute_power writes for frame x and image row y - the same geometry, limits, statuses, channel
 * mode and row order as for the track above - and threshold[y] one double per image row:
 *     hit(x, y)            = power[x][y] >= threshold[y]       numpy's >=: A NaN ON EITHER SIDE IS NO HIT
 *     rows[y]              = the number of x in [0, width) with hit(x, y)            uint32_t rows[n]
 *     frames[b * width + x] = the number of y in [y0_b, y1_b) with hit(x, y)         uint32_t frames[count * width], BAND-MAJOR
 * The bands are exactly the band-power series' bands: a HOST array int32_t bands[2 * count] of half-open row ranges with 0 <= y0 <= y1
 * <= n, read before the call returns; 0 <= count <= SP_MAX_BANDS; bands may overlap and may be empty (an empty band counts 0).  `rows`
 * is over all n rows and needs no bands.  A threshold of -inf, or any negative one, is reached by every value that is not a NaN; one of
 * +inf only by +inf; -0.0 is +0.0.
 * Either output may be NULL and is not written then; both NULL is SP_ERR_INVALID_ARG.  A non-NULL `rows` is ALWAYS written: a request
 * of no frames (width == 0, or a capture shorter than n, whose frames are NaN) gives n zeros.  `frames` is written when it is non-NULL
 * and count > 0 && width > 0.  SP_ERR_INVALID_ARG also for: a NULL threshold or one that is not 8-byte aligned, an output that is not
 * 4-byte aligned, a band outside 0 <= y0 <= y1 <= n, count outside 0 .. SP_MAX_BANDS, bands == NULL with count > 0.  width < 2^31 and n
 * <= SP_MAX_N, so no count overflows 32 bits.  Only plans of the sample detector are accepted: a peak plan returns SP_ERR_UNSUPPORTED.
 * The counts are the same for both layouts and do not depend on gain, range, LUT or block_norm, NOR ON THE CU COUNT, THE WINDOW OR THE
 * CHUNKING OF A HOST-FED REQUEST: integer adds commute.
 * How: no floating-point compare or add anywhere.  A threshold becomes a key once - all ones for a NaN, 0 for a negative one, else its
 * bit pattern without the sign bit - and a value hits when its key is no NaN's and not below that (csrc/sp_occupancy_core.h, the one
 * place the decision is made, for the kernel and for sp_debug_occupancy; the keys are the track's).  Both outputs are zeroed on the
 * stream (two memsets) and ONE launch behind every block of frames reads the plane once for both: no workspace of the context.  The
 * kernel's tile is SP_OCCUPANCY_TILE_ROWS rows: up to that n a frame count gets one add, beyond it one per tile its band touches.
 *
 * sp_power_occupancy: the counts over a frame-major plane double[width * n] the caller holds on the device; the companion of
 *   sp_power_tracks.  Asynchronous on the context's stream, no workspace of the context and no request number: a stream that is being
 *   captured is not refused.  1 <= n <= SP_MAX_N (any n, not only powers of two), width >= 0; d_power (non-NULL when width > 0) and
 *   d_threshold 8-byte aligned device pointers.  The values must not be negative: the sign bit of a value is not looked at.
 * sp_plan_execute_occupancy: device operands (d_threshold too), asynchronous.  The plane is never held whole: it passes block by
 *   block through the mean's window (sp_context_set_mean_window applies) and each block's hits are added behind it.  The checks are
 *   sp_plan_execute_power's, then the bands', then the threshold's and the outputs'.  No request number: the call may be interleaved
 *   with sp_plan_execute / _power / _mean / _bandpower / _track on one context without a synchronisation.
 * sp_render_occupancy: host buffers (threshold: n doubles on the host), synchronous, the plan cached as by sp_render.  The samples
 *   travel as for sp_render_track; the thresholds are uploaded in front of the first chunk and `rows` and `frames` come back in one
 *   copy each.  There is no dB form: counts are not powers.
 * sp_plan_occupancy_kernel_name_for: "frames_power+occupancy" or "scratch_power+occupancy", following sp_plan_power_kernel_name_for.
 * sp_debug_occupancy: (tests, no device needed) *count = the hits among the rows [y0, y1) of one frame's `n` values against `n`
 *   thresholds through the host side of the code the kernel runs.  SP_ERR_INVALID_ARG for a NULL argument, n < 1 or a band outside
 *   0 <= y0 <= y1 <= n.
 * Out of scope: thresholds in dB (the dB formula has no bit-exact inverse), hysteresis and burst lists, accumulation over successive
 * captures, peak plans, batches, groups, sharding.py, and the count fused into the frame loop.
 */
#define SP_OCCUPANCY_TILE_ROWS 4096
int sp_power_occupancy(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const double *d_threshold, const int32_t *bands,
                       int32_t count, uint32_t *d_rows, uint32_t *d_frames);
int sp_plan_execute_occupancy(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const double *d_threshold,
                              const int32_t *bands, int32_t count, uint32_t *d_rows, uint32_t *d_frames);
int sp_render_occupancy(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const double *threshold,
                        const int32_t *bands, int32_t count, uint32_t *rows, uint32_t *frames);
const char *sp_plan_occupancy_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);
int sp_debug_occupancy(const double *values, const double *thresholds, int32_t n, int32_t y0, int32_t y1, uint32_t *count);

/*
 * Percentile traces: order statistics per image row - the median or a low percentile of a row as its noise floor (the 20 %-level of
 * ITU-style occupancy measurements), a high one (p90, p99) as a max-hold that one glitch frame does not own.  With power[x][y] the
 * value sp_plan_execute_power writes for frame x and image row y - the same geometry, limits, statuses, channel mode and row order as
 * for the occupancy counts above:
 *     out[r * n + y] = element ranks[r] of row y's `width` values power[0 .. width)[y] SORTED ASCENDING BY KEY     double out[count * n], RANK-MAJOR
 * The key of a value is its bit pattern with the sign bit cleared, compared as an unsigned integer (csrc/sp_track_core.h): values
 * below +inf, +inf behind them, EVERY NaN BEHIND +inf.  For a value that is not a NaN the reply is the value's bits with the sign bit
 * cleared - on the library's own plane bit for bit np.sort(plane[:, y])[k]; where element k is a NaN the reply is the one NaN
 * 0x7ff8000000000000 (spt::kNanBits).  Equal values are indistinguishable, so ties need no rule.
 * The ranks are a HOST array int32_t ranks[count], read before the call returns, 1 <= count <= SP_MAX_RANKS; they may repeat and need
 * not be ordered.  When width > 0 every rank must satisfy 0 <= k < width: else SP_ERR_INVALID_ARG before the device is touched.
 * SP_ERR_INVALID_ARG also for count < 1, count > SP_MAX_RANKS, a NULL `ranks` and a NULL or not 8-byte aligned `out`.  width == 0 writes
 * count * n NaNs and checks no rank, as the mean writes n NaNs.  n <= SP_MAX_N.  Only plans of the sample detector are accepted: a
 * peak plan returns SP_ERR_UNSUPPORTED.
 * The same bits come out for both layouts; they do not depend on gain, range, LUT or block_norm, NOR ON THE CU COUNT, THE WINDOW OR
 * THE CHUNKING OF A HOST-FED REQUEST: an order statistic does not depend on the order in which the values arrive.
 * sp_quantile_rank: the rank of a quantile, in one place: floor(q * (width - 1)) in IEEE double for 0 <= q <= 1 and width >= 1, -1
 *   otherwise (a NaN q included).  This is numpy's method='lower': np.quantile(x, q, method='lower') == np.sort(x)[rank]; the median
 *   of an even width is the lower one.  Every layer above turns a q into a rank through this function and nothing else.
 * MEMORY: unlike every other consumer this one keeps the request's WHOLE plane, as keys, in a workspace of the context: 8 * n * width
 *   bytes.  The mean's window bounds the block of the plane that is being rendered, not this.  A request whose workspace cannot be had
 *   returns SP_ERR_NOMEM.  The workspace grows as the mean's does: to the largest request so far, never shrunk, freed with the context.
 * How: behind every block of frames one launch transposes it into the workspace u64 keys[n][width]; behind the last block one launch, a
 *   workgroup per row, selects all the ranks by an MSB-first radix select on the keys (csrc/sp_quantile_core.h, the one place the
 *   decision is made, for the kernel and for sp_debug_quantile).  A row of up to SP_QUANTILE_LDS_VALUES keys is held in LDS for all
 *   passes; a longer row streams from the workspace on every pass.
 *
 * sp_power_quantile: the ranks over a frame-major plane double[width * n] the caller holds on the device; the companion of
 *   sp_power_occupancy.  Asynchronous on the context's stream.  1 <= n <= SP_MAX_N (any n), width >= 0; d_power (non-NULL when width >
 *   0) and d_out 8-byte aligned device pointers.  The values must not be negative: the sign bit of a value is not looked at.
 * sp_plan_execute_quantile: device operands, asynchronous.  The checks are sp_plan_execute_power's, then the ranks', then the
 *   output's.  No request number: the call may be interleaved with sp_plan_execute / _power / _mean / _bandpower / _track / _occupancy
 *   on one context without a synchronisation.
 * sp_render_quantile: host buffers, synchronous, the plan cached as by sp_render.  The samples travel as for sp_render_mean; db != 0
 *   converts the reply through sp_plan_power_to_db's kernel before the one copy back.
 * sp_plan_quantile_kernel_name_for: "frames_power+quantile" or "scratch_power+quantile", following sp_plan_power_kernel_name_for.
 * sp_debug_quantile: (tests, no device needed) *out = the reply of element `rank` of `count` values through the host side of the code
 *   the kernel runs.  SP_ERR_INVALID_ARG for a NULL argument, count < 1 or a rank outside 0 <= rank < count.
 * Out of scope: interpolated quantiles and other rank rules, peak plans, batches, groups, sharding.py, a select that re-renders
 * instead of keeping keys, accumulation over successive captures, and the gather fused into the frame loop.
 */
#define SP_MAX_RANKS 16
#define SP_QUANTILE_LDS_VALUES 16384
int sp_power_quantile(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *ranks, int32_t count, double *d_out);
int sp_plan_execute_quantile(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *ranks, int32_t count,
                             double *d_out);
int sp_render_quantile(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t db,
                       const int32_t *ranks, int32_t count, double *out);
const char *sp_plan_quantile_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);
int32_t sp_quantile_rank(int32_t width, double q);
int sp_debug_quantile(const double *values, int32_t count, int32_t rank, double *out);

/*
 * Burst lists: hysteresis pulse edges per band - when a transmitter switches on and off and for how long, the pulse widths and gaps
 * of an OOK or FSK capture that one otherwise reads off the spectrogram by eye.  With s[b][x] the value sp_plan_execute_bandpower
 * writes for band b and frame x - the same bands (a HOST array of `count` pairs, 0 <= count <= SP_MAX_BANDS), geometry, limits,
 * statuses, channel mode and bits as for the band-power series above - and two thresholds per band, hi[b] and lo[b], HOST arrays of
 * `count` doubles read before the call returns, every frame of a band is one of
 *     SET     s >= hi, as numpy compares
 *     RESET   s < lo, as numpy compares
 *     HOLD    anything else: lo <= s < hi, and EVERY NaN - a NaN is neither SET nor RESET
 * and a Schmitt trigger per band runs along the frames.  It STARTS OFF in front of frame 0.  After frame x it is ON if the last frame
 * at or before x that is not HOLD is a SET, and OFF if that frame is a RESET or there is none.  A burst is a maximal run of ON frames
 * [start, end); a burst that is still ON behind the last frame has end = width.  The reply:
 *     counts[b]           = the TOTAL number of bursts of band b                                      uint32_t counts[count]
 *     edges[b][2 i]       = start, edges[b][2 i + 1] = end of burst i, ascending in time,
 *                           for i < min(counts[b], max_bursts); EVERY SLOT BEHIND THAT IS -1          int32_t edges[count][2 * max_bursts]
 * Either output may be NULL and is not touched then; `edges` is also absent with max_bursts == 0.  Both absent: SP_ERR_INVALID_ARG.
 * Both are 4-byte aligned.  max_bursts >= 0 and 2 * max_bursts * count must fit 31 bits.  counts[b] > max_bursts says the list is cut.
 * The thresholds become keys once (csrc/sp_occupancy_core.h, threshold_key): a negative one and -0.0 are key 0, so a negative lo
 * never resets and a negative hi is reached by every value that is not a NaN.  A NaN hi or lo is SP_ERR_INVALID_ARG, and so is
 * lo_key > hi_key, before the device is touched; lo == hi is a plain threshold.  Also SP_ERR_INVALID_ARG: what the band-power series
 * refuses of its bands, a NULL hi or lo with count > 0, max_bursts < 0.  Only plans of the sample detector are accepted: a peak plan
 * returns SP_ERR_UNSUPPORTED.  width == 0 or count == 0: a non-NULL counts gets `count` zeros and edges all -1.
 * The same words come out for both layouts; they do not depend on gain, range, LUT or block_norm, NOR ON THE CU COUNT, THE WINDOW OR
 * THE CHUNKING OF A HOST-FED REQUEST, although a Schmitt trigger is a recurrence along time: the series is written whole first, and a
 * run of frames is known to what follows it by a summary that combines associatively (csrc/sp_burst_core.h, the one place the decision
 * is made, for the kernels and for sp_debug_bursts; no floating-point compare).
 * MEMORY: the context keeps the band series, 8 * count * width bytes, and 16 bytes per band and segment of SP_BURST_SEGMENT_FRAMES
 *   frames in a workspace that grows to the largest request so far, is never shrunk and is freed with the context; SP_ERR_NOMEM
 *   where it cannot be had.
 * How: behind every block of frames the band-power series' launch writes the block's columns of the workspace series; behind the last
 *   block three launches: a summary per segment and band, one wave per band that scans the summaries (the state in front of every
 *   segment, the bursts started before it, the total), and the first grid again, which stores the edges with plain stores - every slot
 *   has one writer.  No workgroup waits for another.  `edges` is filled with 0xFF bytes on the stream in front of all that.
 *
 * sp_plan_execute_bursts: device operands, asynchronous on the context's stream, capturable.  The checks are
 *   sp_plan_execute_bandpower's, then the thresholds', then the outputs'.  No request number: the call may be interleaved with
 *   sp_plan_execute / _power / _mean / _bandpower / _track / _occupancy / _quantile on one context without a synchronisation.
 * sp_power_bursts: the bursts of a frame-major plane double[width * n] the caller holds on the device; the companion of
 *   sp_power_bands.  Asynchronous.  n >= 1 (any n), width >= 0; d_power (non-NULL when width > 0 and count > 0) 8-byte aligned.
 * sp_series_bursts: the three launches alone on a band-major device series double[count * width] the caller holds, sp_power_bands'
 *   reply for example: band b's frames at d_series + b * width.  0 <= count <= SP_MAX_BANDS, width >= 0, d_series 8-byte aligned and
 *   non-NULL when count * width > 0.  The values are read by key: the sign bit of a value is not looked at.  Asynchronous.
 * sp_render_bursts: host buffers, synchronous, the plan cached as by sp_render.  The samples travel as for sp_render_bandpower; the
 *   reply comes back in two copies.  There is no dB form: the thresholds are powers.
 * sp_plan_bursts_kernel_name_for: "frames_power+bursts" or "scratch_power+bursts", following sp_plan_power_kernel_name_for.
 * sp_debug_bursts: (tests, no device needed) one band on the host through the host side of the code the kernels run: `width` >= 0
 *   values, the thresholds hi and lo, *count_out = the total and edges_out[2 * max_bursts] the list.  Either output may be NULL, not
 *   both; the refusals of the thresholds, of max_bursts and of the outputs' alignment are those above.
 * Out of scope: a minimum burst width or gap, peak plans, batches, groups, sharding.py, a dB form.  (The energy and the peak of a
 *   burst: "Burst measurements", below.)
 */
#ifndef SP_BURST_SEGMENT_FRAMES   /* (a compile-time knob for tools/burst_bench.py's variants only) */
#define SP_BURST_SEGMENT_FRAMES 2048
#endif
int sp_plan_execute_bursts(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                           const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges);
int sp_power_bursts(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, const double *hi,
                    const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges);
int sp_series_bursts(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const double *hi, const double *lo,
                     int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges);
int sp_render_bursts(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                     int32_t count, const double *hi, const double *lo, int32_t max_bursts, uint32_t *counts, int32_t *edges);
const char *sp_plan_bursts_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);
int sp_debug_bursts(const double *values, int32_t width, double hi, double lo, int32_t max_bursts, uint32_t *count_out, int32_t *edges_out);

/*
 * Exact lagged covariances of band-power series: how a frame relates to another frame - the autocovariance of a channel over lag (its
 * symbol or repetition period) and the cross-covariance of two channels (FSK mark against space, a hopper, a wide-band interferer).
 * Bit-exact like the variance: a band-power series sits on a pedestal and N * sum(a b) - sum(a) * sum(b) is the small difference of two
 * huge terms, noise in floating point and one integer here.
 * With s[b][x] the value sp_plan_execute_bandpower writes for band b and frame x - the same bands (a HOST array of `count` pairs,
 * 0 <= count <= SP_MAX_BANDS), geometry, limits, statuses, channel mode and bits as for the band-power series above - `pairs` is a HOST
 * array of `npairs` index pairs (ia, ib) into the bands, read before the call returns, 0 <= npairs <= SP_MAX_LAG_PAIRS; ia == ib is an
 * autocovariance.  1 <= lags <= SP_MAX_LAGS.  N = width - lags + 1 where that is at least 1, else N = 0: the number of terms, THE SAME
 * FOR EVERY LAG (the fixed window: every lag sees equally many frames).  The reply is double[3][npairs][lags]; for pair p = (a, b) -
 * a = s[ia], b = s[ib] - and lag l in [0, lags):
 *     out[0][p][l] = RN( P ),               P = sum over x in [0, N) of a[x] * b[x + l]
 *     out[1][p][l] = RN( N * P - A * B ),   A = sum over x in [0, N) of a[x],   B = sum over x in [0, N) of b[x + l]
 *     out[2][p][l] = RN( B )
 * Every product, sum and the difference is the EXACT real number; RN is one IEEE-754 round-to-nearest-even to f64, INTO THE DENORMAL
 * RANGE where the value lies there and to +-inf past DBL_MAX.  out[1] is SIGNED: a negative value carries the sign bit (also where it rounds to zero), an exact
 * zero is +0.0, never -0.0.  out[1] is N^2 times the lag-l covariance; the covariance itself is one IEEE divide and stays with the caller.  A is
 * out[2][q][0] of any pair q whose second index is ia.  In Python, with Fractions (OverflowError read as the infinity of the value's
 * sign): float(sum(fa[x] * fb[x + l] for x in range(N))), float(N * P - A * B), float(sum(fb[l:l + N])).
 * SPECIAL VALUES follow the mean's rule per (p, l) on the frames the window touches, a[0 .. N) and b[l .. l + N): a NaN among them gives
 * NaN in all three arrays of that (p, l) (A NaN IS ANY NaN); otherwise a +inf among them gives +inf in all three.  The rule goes by
 * presence, not by arithmetic: 0 * inf is marked +inf.  A NaN at b[N + l0 - 1] marks exactly the lags l >= l0.
 * N == 0 (width == 0 too) writes 3 * npairs * lags times +0.0.  npairs == 0 or count == 0 writes nothing and returns SP_OK.
 * The values must not be negative: the sign bit of a value is not looked at.  The reply depends on nothing but the series: NOT ON gain,
 * range, LUT or block_norm, NOR ON THE CU COUNT, THE DEAL OF TERMS TO WORKGROUPS, THE WINDOW OR THE CHUNKING OF A HOST-FED REQUEST
 * (integer adds commute).
 * SP_ERR_INVALID_ARG, before the device is touched: what the band-power series refuses of its bands, an index outside [0, count),
 * npairs or lags outside their limits, pairs == NULL with npairs > 0, a NULL or misaligned (8 bytes) output with npairs > 0.  Only plans
 * of the sample detector are accepted: a peak plan returns SP_ERR_UNSUPPORTED.
 * MEMORY: the context keeps the band series, 8 * count * width bytes, and 1600 bytes per (pair, lag) plus 528 per pair (26 MB at 16
 *   pairs of 1024 lags) in a workspace of its own that grows to the largest request so far, is never shrunk and is freed with the
 *   context; SP_ERR_NOMEM where it cannot be had.  The cells are zeroed on the stream by every request.
 * How: csrc/sp_lagcov_core.h.  Behind every block of frames the band-power series' launch writes the block's columns of the workspace
 *   series (the burst lists' way: the series is whole and independent of the window before anything is correlated); behind the last
 *   block k_lagcov_accumulate - a workgroup per pair, band of 32 lags and piece of the terms; b's three 32-bit pieces go to 66 cells and
 *   the product's five to 132, integer adds only - and k_lagcov_finish, which forms N * P and A * B digit by digit, subtracts with a
 *   borrow, takes the two's complement where the last borrow says the difference is negative, and rounds once.
 *
 * sp_plan_execute_lagcov: device operands, asynchronous on the context's stream.  The checks are sp_plan_execute_bandpower's, then the
 *   pairs', the lags' and the output's.  No request number: the call may be interleaved with sp_plan_execute / _power / _mean /
 *   _bandpower / _variance on one context without a synchronisation.
 * sp_power_lagcov: of a frame-major plane double[width * n] the caller holds on the device; the companion of sp_power_bands.
 *   Asynchronous.  n >= 1 (any n), width >= 0; d_power (non-NULL when width > 0) 8-byte aligned.
 * sp_series_lagcov: the two launches alone on a band-major device series double[count * width] the caller holds, sp_power_bands' reply
 *   for example: band b's frames at d_series + b * width.  0 <= count <= SP_MAX_BANDS, width >= 0, d_series 8-byte aligned and non-NULL
 *   when count * width > 0.  Asynchronous.
 * sp_render_lagcov: host buffers, synchronous, the plan cached as by sp_render.  The samples travel as for sp_render_bandpower and the
 *   3 * npairs * lags doubles come back in one copy.  There is no dB form: a covariance has a sign.
 * sp_plan_lagcov_kernel_name_for: "frames_power+lagcov" or "scratch_power+lagcov", following sp_plan_power_kernel_name_for.
 * sp_debug_lagcov: (tests, no device needed) out[3][lags] of the series a and b of `width` >= 0 non-negative values each, through the
 *   host side of the code the kernels run.  A negative value, -0.0 or -inf, lags outside 1 .. SP_MAX_LAGS or a NULL out returns
 *   SP_ERR_INVALID_ARG and writes nothing.
 * sp_debug_lagcov_launch: (tests, no device needed) the grid of the accumulation behind `terms` >= 1 terms of npairs >= 1 pairs and
 *   `lags` lags on a part with cu_count CUs: out[] receives 3 int64 words - npairs * ceil(lags / 32) bands, the pieces the terms are cut
 *   into (about 6 workgroups per CU, no piece below 32 terms) and the terms per piece (the last piece may be shorter).  *used = words
 *   needed (SP_ERR_INVALID_ARG if capacity is smaller).
 * Out of scope: the Node addon (its export table is pinned), peak plans, batches, groups and sharding.py, negative lags (swap the pair),
 *   more than SP_MAX_LAGS lags or an FFT-based form, the per-window variance of b, a correlation coefficient computed on the device, and
 *   the product fused into the band-sum launch.
 */
#define SP_MAX_LAG_PAIRS 16
#define SP_MAX_LAGS 1024
int sp_series_lagcov(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const int32_t *pairs, int32_t npairs,
                     int32_t lags, double *d_out);
int sp_power_lagcov(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count,
                    const int32_t *pairs, int32_t npairs, int32_t lags, double *d_out);
int sp_plan_execute_lagcov(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                           const int32_t *pairs, int32_t npairs, int32_t lags, double *d_out);
int sp_render_lagcov(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                     int32_t count, const int32_t *pairs, int32_t npairs, int32_t lags, double *out);
const char *sp_plan_lagcov_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);
int sp_debug_lagcov(const double *a, const double *b, int32_t width, int32_t lags, double *out);
int sp_debug_lagcov_launch(int32_t npairs, int32_t lags, int64_t terms, int32_t cu_count, int64_t *out, size_t capacity, size_t *used);

/*
 * Burst measurements: exact energy and peak per burst - how strong each pulse of the burst lists above is, the level and the peak a
 * pulse analyser prints beside width and gap, without copying the band series to the host.  The inputs are those of the burst lists:
 * bands, count, hi[], lo[], max_bursts; s[b][x] is the band-power series and the bursts [start, end) of band b are EXACTLY those of
 * sp_plan_execute_bursts, the open burst with end = width included.  For every listed burst i < min(counts[b], max_bursts):
 *     energy[b][i]  = RN(exact sum of s[b][x] for x in [start, end)): Python's math.fsum of the burst's frames, rounded ONCE.  The
 *                     rule of the specials is spx::apply_specials': any NaN frame gives the NaN 0x7ff8000000000000 (a burst may
 *                     hold NaN frames: a NaN is HOLD), otherwise any +inf frame gives +inf, and a finite sum beyond DBL_MAX gives
 *                     +inf.  Values are read by key: the sign bit is not looked at.                   double energy[count][max_bursts]
 *     peak[b][i]    = the largest s[b][x] of the burst that is not a NaN, as a key (the sign bit cleared).  Powers are ordered as
 *                     unsigned integers; there is no floating-point compare.                           double peak[count][max_bursts]
 *     peak_at[b][i] = the EARLIEST frame of the burst that holds peak[b][i].  A burst's first frame is a SET, so it is not a NaN:
 *                     every burst has a peak.                                                          int32_t peak_at[count][max_bursts]
 * beside counts[count] and edges[count][2 * max_bursts] as the burst lists reply them.  Any output may be NULL and is not touched
 * then; a per-burst output (edges, energy, peak, peak_at) with max_bursts == 0 counts as absent; all absent: SP_ERR_INVALID_ARG.
 * EVERY SLOT BEHIND min(counts[b], max_bursts) HOLDS 0xFF BYTES: -1 in the int arrays, the all-ones NaN pattern in the double arrays.
 * Bursts cut off by max_bursts are not measured.  energy and peak are 8-byte aligned, the int arrays 4-byte aligned.  The refusals are
 * those of the burst lists, in the same order; a peak plan returns SP_ERR_UNSUPPORTED.  width == 0 or count == 0: zeros in counts
 * and the fill elsewhere.  The reply does not depend on the CU count, the window, the chunking of a host-fed request or
 * SP_BURST_SEGMENT_FRAMES: the energy's cells are added with integer adds and the peak is folded in a strict total order - the
 * larger key, of equal keys the smaller frame (csrc/sp_pulse_core.h, the one place the decision is made, for the kernels and for
 * sp_debug_pulses) - so neither depends on the order of the frames.
 * MEMORY: beside the burst lists' workspace the context keeps 8 * 68 * count * max_bursts bytes of cells (68 = spx::kSlots, csrc/
 *   sp_exact_sum.h), 8 * count * max_bursts bytes of peak keys and 4 * count bytes of counts in a workspace of its own that grows to
 *   the largest request so far, is never shrunk and is freed with the context; SP_ERR_NOMEM where it cannot be had.  max_bursts is
 *   what sizes it, not the number of bursts found.
 * How: the three burst launches run first, unchanged.  Behind them the workspace is zeroed and, on the burst kernels' grid (segments,
 *   bands), one launch adds every ON frame's pieces to its burst's cells and folds its key into the burst's peak key with integer
 *   atomics whose results are not used - the burst that enters a segment and the last one that starts in it gather in LDS first, so a
 *   burst of a million frames does not hammer one address; a second launch on the same grid puts the earliest frame whose key is the
 *   peak key into peak_at with an UNSIGNED atomic minimum (the -1 fill is the largest unsigned word); a third, a thread per listed
 *   burst, rounds the cells once and stores energy and peak with plain stores.  No workgroup waits for another.  The per-burst
 *   outputs are filled with 0xFF bytes on the stream in front of all that.
 *
 * sp_plan_execute_pulses: device operands, asynchronous on the context's stream, capturable once the workspaces have their sizes.  No
 *   request number: the call may be interleaved with the other sp_plan_execute_* on one context without a synchronisation.
 * sp_power_pulses: on a frame-major plane double[width * n] of the device, as sp_power_bursts.  Asynchronous.
 * sp_series_pulses: the burst launches and the measurement alone on a band-major device series double[count * width], the companion of
 *   sp_series_bursts with its limits.  Asynchronous.
 * sp_render_pulses: host buffers, synchronous, as sp_render_bursts; the reply comes back in up to five copies.
 * sp_plan_pulses_kernel_name_for: "frames_power+pulses" or "scratch_power+pulses", following sp_plan_power_kernel_name_for.
 * sp_debug_pulses: (tests, no device needed) one band on the host through the host side of the code the kernels run; the outputs
 *   are *count_out, edges_out[2 * max_bursts] and energy_out, peak_out, peak_at_out of max_bursts slots each, any of them NULL.
 * Out of scope: the mean (energy / (end - start)) and the dB forms stay with the caller; the frequency of a burst is sp_*_track's
 *   rows[b][peak_at], a gather the caller does; a minimum burst width or gap, peak plans, batches, groups, sharding.py, a per-burst row.
 */
int sp_plan_execute_pulses(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const int32_t *bands, int32_t count,
                           const double *hi, const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges, double *d_energy,
                           double *d_peak, int32_t *d_peak_at);
int sp_power_pulses(sp_context *ctx, const double *d_power, int32_t n, int32_t width, const int32_t *bands, int32_t count, const double *hi,
                    const double *lo, int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges, double *d_energy, double *d_peak,
                    int32_t *d_peak_at);
int sp_series_pulses(sp_context *ctx, const double *d_series, int32_t count, int32_t width, const double *hi, const double *lo,
                     int32_t max_bursts, uint32_t *d_counts, int32_t *d_edges, double *d_energy, double *d_peak, int32_t *d_peak_at);
int sp_render_pulses(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const int32_t *bands,
                     int32_t count, const double *hi, const double *lo, int32_t max_bursts, uint32_t *counts, int32_t *edges, double *energy,
                     double *peak, int32_t *peak_at);
const char *sp_plan_pulses_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);
int sp_debug_pulses(const double *values, int32_t width, double hi, double lo, int32_t max_bursts, uint32_t *count_out, int32_t *edges_out,
                    double *energy_out, double *peak_out, int32_t *peak_at_out);

/*
 * Averaged spectrogram: exact block means over frames - the average (RMS) detector of a spectrum analyser, the third beside the sample
 * detector and the peak hold.  A column is the mean power of all the frames it stands for: noise averages down, a weak carrier comes out
 * of it, and one glitch frame does not own the column.  It is the time-resolved Welch spectrogram between the two extremes the library
 * already has: with group == 1 it is the power plane, with group >= width it is the mean-power trace.
 * With power[x][y] the value sp_plan_execute_power writes for frame x and image row y - the same geometry, limits, statuses, channel
 * mode and row order y = i <= n/2 ? n/2 - i : n/2 + n - i (worker.js:90) - and `group` an int32_t >= 1, the frames per column:
 *     columns = sp_blockmean_columns(width, group) = ceil(width / group), computed in 64 bits; 0 for width == 0
 *     column c covers the frames [c * group, min((c + 1) * group, width)); count_c is their number: only the last column can be short
 *     out[c * n + y] = RN( sum over the column's frames x of power[x][y] ) / (double)count_c
 * The sum is the EXACT real-number sum, RN one IEEE-754 round-to-nearest-even to f64, the division one correctly rounded f64 division:
 * the rule of the mean-power trace.  In Python: math.fsum(plane[c * group : (c + 1) * group, y]) / count_c, OverflowError read as +inf.
 * A column and row with a NaN in any of its frames is the NaN 0x7ff8000000000000; otherwise one with +inf in any frame is +inf; a
 * finite sum from 2^1024 - 2^970 up gives +inf; a column of zeros gives +0.0.
 * `out` is double[columns][n], FRAME-MAJOR like the plane, 8-byte aligned: it is itself a power plane of `columns` frames, and every
 * sp_power_* consumer runs on it unchanged.  It is the same for both layouts and does not depend on gain, range, LUT or block_norm.
 * Refusals, in this order: a NULL or misaligned `out` with columns > 0 is SP_ERR_INVALID_ARG; group < 1 is SP_ERR_INVALID_ARG; a peak
 * plan is SP_ERR_UNSUPPORTED.  width == 0 writes nothing and returns SP_OK.
 * THE REPLY DOES NOT DEPEND ON THE CU COUNT, THE WINDOW, THE CHUNKING OF A HOST-FED REQUEST OR THE PATH SPLIT BELOW: every path adds the
 * same integers into the mean's cells (csrc/sp_exact_sum.h) and rounds once.  Hence, bit for bit: group == 1 gives the power plane
 * (every NaN as the one NaN above), and group >= width gives the n values of sp_*_mean.
 * How: a plane consumer receives the request's frames in runs that end wherever a window block or a chunk ends.  A run is cut
 * (csrc/sp_blockmean_core.h, the one place the decision is made) into a head that continues a column an earlier run began, a body of
 * whole columns and a tail that begins a column a later run finishes.  Body columns of group <= direct_max frames are made by ONE
 * launch of k_blockmean, the DIRECT path: a workgroup owns 64 rows and one column at a time, adds the column's frames into cells in LDS
 * and finishes them there - no workspace, no global atomic.  Head, tail and larger columns are CARRIED: added by the mean's own launches
 * into the context's mean workspace ((66 + 2) * 8 * n bytes), which is cleared on the stream where a column begins and finished where
 * it ends; a column of group == width is the mean-power trace's launches, one for one.
 *
 * sp_blockmean_columns: (pure host arithmetic) ceil(width / group); 0 where width <= 0 or group < 1.
 * sp_power_blockmean: the block means of a frame-major plane double[width * n] the caller holds on the device; the companion of
 *   sp_power_mean.  Asynchronous on the context's stream, no request number: a stream that is being captured is not refused once the
 *   workspace has its size.  n >= 1 (any n), width >= 0; both pointers 8-byte aligned, d_power non-NULL when width > 0.  The values must
 *   not be negative: the sign bit of a value is not looked at.
 * sp_plan_execute_blockmean: device operands, asynchronous.  The plane is never held whole: it passes block by block through the mean's
 *   window (sp_context_set_mean_window applies).  The checks are the output's and the group's, then sp_plan_execute_power's.  No
 *   request number: the call may be interleaved with the other sp_plan_execute_* on one context without a synchronisation.
 * sp_render_blockmean: host buffers, synchronous, the plan cached as by sp_render.  The samples travel as for sp_render_mean - a packed
 *   upload where stride > n, chunks of frames where the request is large - and the columns * n doubles come back in ONE copy behind the
 *   last chunk, converted on the device first when db != 0: sp_plan_power_to_db of the means, the dB of the mean and NOT the mean of the
 *   dB values.  The reply waits on the device for that copy, 8 * columns * n bytes of the context's small-reply buffer: where they
 *   cannot be had the call returns SP_ERR_NOMEM and the reply is not cut.  sp_context_last_upload_bytes / _last_chunks report as before.
 * sp_plan_blockmean_kernel_name_for: "frames_power+blockmean" or "scratch_power+blockmean", following sp_plan_power_kernel_name_for.
 * sp_context_set_blockmean_direct_max: (tests) direct_max in frames, 1 ... 2^31 - 1; 0 restores the built default,
 *   SP_BLOCKMEAN_DIRECT_FRAMES.  It changes speed only, never a bit.
 * sp_debug_blockmean: (tests, no device needed) the reply of `width` frames of n values through the host side of the code the kernels
 *   run, one spx::Accumulator per column and row.  SP_ERR_INVALID_ARG for n < 1, width < 0, group < 1, a NULL array with width > 0 and
 *   a negative value, -0.0 or -inf.
 * sp_debug_blockmean_split: (tests, no device needed) what becomes of the run [x_base, x_base + frames) of a request of `width` frames,
 *   from the function the consumer calls: out[] receives 6 int64 words - the frames of the head, of the body and of the tail (they sum to
 *   `frames`), the body's first column, its number of columns, and 1 where the body goes to k_blockmean (direct_max 0: the built
 *   default).  *used = words needed (SP_ERR_INVALID_ARG if capacity is smaller, or 0 <= x_base, 0 <= frames, x_base + frames <= width,
 *   group >= 1 does not hold).
 *
 * sp_debug_blockmean_launch: (tests, no device needed) k_blockmean's grid for the whole columns of `frames` >= 1 frames of n rows on a
 *   part with cu_count CUs: out[] receives 3 int64 words - the bands of 64 rows, the pieces the columns are cut into (about 8
 *   workgroups per CU where there are columns enough, 65535 at the most) and the columns per piece.  *used as above.
 *
 * sp_plan_power_to_index: colours a plane as the frame loop colours its own pixels.  d_power is double[width * n], frame-major, n the
 *   plan's: a power plane, a block-mean plane or anything else of that shape.  d_index[j] = gray of lib/worker.js:105-117 of the value,
 *   with the plan's gain, range, block_norm and LUT length, at the pixel position "Indexed image replies" defines for frame x and row
 *   y in the plan's layout; sp_index_to_rgba makes RGBA of it.  On a sample plan's own plane it is sp_plan_execute_index's image byte
 *   for byte.  The index is decided against the plan's colour edges by integer comparison of bit patterns (csrc/sp_blockmean_core.h):
 *   0 and NaN take index 0, +inf takes the last index.  The sign bit of a value is not looked at.  Asynchronous on the context's stream,
 *   ONE launch, no workspace and no request number: capturable.  Peak plans are accepted: it only colours.  lut_len > 256 is
 *   SP_ERR_UNSUPPORTED; with width > 0 a NULL pointer or a d_power that is not 8-byte aligned is SP_ERR_INVALID_ARG; width == 0 queues
 *   nothing.
 * sp_debug_gray_index: (tests, no device needed) out[k] = that index of values[k] for a plan of these four parameters, through the host
 *   side of the code the kernel runs; 1 <= lut_len <= 256.
 * Out of scope: the Node addon (its export table is pinned, as for the burst lists), peak plans, batches, groups, sharding.py,
 * overlapping or exponentially weighted averages, and the accumulation fused into the frame loop.
 */
#define SP_BLOCKMEAN_DIRECT_FRAMES 1024
int32_t sp_blockmean_columns(int32_t width, int32_t group);
int sp_power_blockmean(sp_context *ctx, const double *d_power, int32_t n, int32_t width, int32_t group, double *d_out);
int sp_plan_execute_blockmean(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, int32_t group, double *d_out);
int sp_render_blockmean(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, int32_t group,
                        int32_t db, double *out);
const char *sp_plan_blockmean_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);
int sp_context_set_blockmean_direct_max(sp_context *ctx, int32_t frames);
int sp_debug_blockmean(const double *values, int32_t n, int32_t width, int32_t group, double *out);
int sp_debug_blockmean_split(int64_t x_base, int64_t frames, int32_t width, int32_t group, int32_t direct_max, int64_t *out, size_t capacity,
                             size_t *used);
int sp_debug_blockmean_launch(int32_t n, int64_t frames, int32_t group, int32_t cu_count, int64_t *out, size_t capacity, size_t *used);
int sp_plan_power_to_index(sp_plan *plan, const double *d_power, int32_t width, uint8_t *d_index);
int sp_debug_gray_index(double block_norm, double gain, double range, int32_t lut_len, const double *values, size_t count, uint8_t *out);

/*
 * Indexed image replies: the picture as ONE colour-index byte per pixel instead of RGBA.
 *     index[j] = gray of lib/worker.js:105-117 (the value `c_hist[gray] += 1` counts), a uint8_t,
 * at the RGBA image's pixel position: j = x + width * y for the spectrogram layout (n rows x width columns) and
 * j = n * (width - 1 - x) + (n - 1 - y) for the waterfall layout (width rows x n columns), y the image row of bin i (worker.js:90).
 * With any LUT, lut_rgb[index[j]] with alpha 255 is sp_render's RGBA of the same request, byte for byte; bincount(index, lut_len) is
 * c_hist exactly; every other reply field (gauges, both histograms, dBfs range) is sp_plan_execute's, bit for bit.  Geometry, limits,
 * statuses, channel mode, both layouts, width 0 and 1, captures shorter than n (NaN frames index 0) and the detector are
 * sp_plan_execute's.  lut_len > 256 returns SP_ERR_UNSUPPORTED: the reference allows longer maps, but a byte cannot hold their index.
 * The image is a quarter of the RGBA image in device memory and on the host link, and a viewer that changes its colour map
 * recolours it (sp_index_to_rgba, or a table lookup of its own) instead of rendering the capture again.
 *
 * sp_plan_execute_index: device operands, asynchronous, sp_plan_execute in every other respect - the same request-number handshake, so
 *   not capturable into a hipGraph (SP_ERR_UNSUPPORTED on a capturing stream), and free to interleave with sp_plan_execute on one
 *   context without a synchronisation in between.  d_reply->rgba must be NULL (SP_ERR_INVALID_ARG otherwise); d_index [width * n] may be
 *   NULL: side outputs only.
 * sp_render_index: host buffers, synchronous, the plan cached as by sp_render.  The capture travels as for sp_render - a packed upload
 *   where stride > n, chunks of frames where the request is large - and the image comes back per chunk at 1 byte per pixel; the
 *   chunking threshold counts the bytes that actually travel.  sp_context_last_upload_bytes reports as before.  reply->rgba must be NULL.
 * sp_index_to_rgba: d_rgba[4 * pixels] = lut_rgb[d_index[i]], alpha 255, on the device and asynchronous on the context's stream;
 *   lut_rgb is a HOST pointer to 3 * lut_len bytes (1 <= lut_len <= 256) that is read before the call returns.  An index >= lut_len
 *   writes (0, 0, 0, 255).  Neither pointer needs any alignment.
 * sp_plan_index_kernel_name_for: "frames_index" - k_frames_index, k_frames' frame loop with a write-out of the tile's bytes - for the
 *   sample plans "frames" covers, or "render_extract" for everything else (n <= 32, n >= 16384, non-finite tapers, peak plans whichever
 *   kernel their request takes, plans forced to kernel 1, and the L/R split with the generic loaders at n <= 256): the request's
 *   ordinary kernel renders through an identity LUT into a temporary RGBA image of the context and a small kernel keeps byte 0 of every
 *   pixel.  sp_plan_force_kernel applies: 1 forces "render_extract", 3 means "frames_index" where it covers the request.
 * sp_plan_debug_index_launch: (tests) sp_plan_debug_launch's 11 words for the launch sp_plan_execute_index would make with the index
 *   image at `index`: word 0 is 5 where k_frames_index runs, and word 8 then tells whether the write-out stores 16-byte pieces (base and
 *   width multiples of 16, image below 4 GiB); on the render_extract path the words are the ordinary render's with word 8 = 0.
 * Out of scope: batches, groups, sharding.py and strip placement (image_width) have no indexed form; no existing call gained a
 * parameter, so none of them refuses anything new.
 */
int sp_plan_execute_index(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, const sp_reply *d_reply, uint8_t *d_index);
int sp_render_index(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, const sp_reply *reply,
                    uint8_t *index);
int sp_index_to_rgba(sp_context *ctx, const uint8_t *d_index, size_t pixels, const uint8_t *lut_rgb, int32_t lut_len, uint8_t *d_rgba);
const char *sp_plan_index_kernel_name_for(const sp_plan *plan, size_t nbytes, int32_t width);
int sp_plan_debug_index_launch(const sp_plan *plan, size_t nbytes, int32_t width, const void *index, int64_t *out, size_t capacity,
                               size_t *used);

/*
 * Persistence spectrum: how often each image row showed each colour index over a request - the frequency x level histogram a real-time
 * spectrum analyser draws as its persistence display.  `density` is uint32_t[n * lut_len], row y at density + y * lut_len:
 *     density[y * lut_len + g] = #{ x in [0, width) : index(x, y) == g }
 * with index(x, y) = gray of lib/worker.js:105-117 for frame x and image row y (worker.js:90): the byte sp_plan_execute_index puts at
 * pixel (x, y).  Row y is image row y of the spectrogram layout and column n - 1 - y of the waterfall layout; the array is the same for
 * both layouts, as the traces are.  Hence, bit for bit: the sum over g of density[y][g] is `width` for every row (the NaN frames of a
 * capture shorter than n count at index 0), and the sum over y of density[y][g] is c_hist[g] of sp_render on the same request.
 * Geometry, limits, statuses, channel mode and detector are sp_plan_execute_index's (peak plans are accepted: a persistence display of
 * held peaks); width 0 gives all zeros; lut_len > 256 returns SP_ERR_UNSUPPORTED.  The counts are integers added with integer atomics:
 * the result does not depend on the deal of pixels to workgroups.  A cell cannot overflow within one request (width < 2^31); with
 * `accumulate` it wraps modulo 2^32.
 *
 * sp_density_from_index (lib/worker.js:105-117, the count alone): the histogram of an index image the caller holds on the device, in the
 *   layout `waterfall` names and at the pixel positions given for sp_plan_execute_index above; the companion of sp_index_to_rgba.
 *   Asynchronous on the context's stream; it carries no request number, so a stream that is being captured is not refused.
 *   accumulate == 0 overwrites d_density, accumulate != 0 adds to it (persistence over successive captures).  A byte >= lut_len is
 *   counted nowhere.  d_index needs no alignment; d_density must be 4-byte aligned, 1 <= lut_len <= 256, n >= 1, width >= 0
 *   (SP_ERR_INVALID_ARG otherwise).  width == 0 zeroes d_density when not accumulating and does nothing otherwise.
 * sp_plan_execute_density (lib/worker.js:105-117 over the frame loop of :68-137): device operands, asynchronous.  The request's index
 *   image is rendered into a workspace of the context - width * n bytes of device memory, grown and never shrunk, ordered on the
 *   stream: that is this call's cost - by sp_plan_execute_index's path (k_frames_index where it covers the request, render_extract
 *   elsewhere; sp_plan_force_kernel applies) and counted into d_density (device pointer, 4-byte aligned: SP_ERR_INVALID_ARG
 *   otherwise).  The same request-number handshake: not capturable into a hipGraph (SP_ERR_UNSUPPORTED on a capturing stream), and
 *   free to interleave with sp_plan_execute / sp_plan_execute_index on one context without a synchronisation.  The render's side
 *   outputs go to a reply record of the context and are not returned.
 * sp_render_density (lib/worker.js:23-156 with the count of :105-117 as its reply): host buffers, synchronous, the plan cached as by
 *   sp_render.  The samples are the only transfer - packed where stride > n, in chunks of frames where the request is large, the
 *   threshold counting the bytes that travel; every chunk's frames are rendered and counted behind its upload, and `density`
 *   (4 * n * lut_len bytes of host memory) comes back in one copy.  sp_context_last_upload_bytes / sp_context_last_chunks report as before.
 * sp_debug_density_launch (lib/worker.js:105-117; tests, no device needed): the counting kernel's decomposition for the frames
 *   [x_begin, x_end) of an image of n rows and `width` frames, from the functions the launch itself calls.  out[] receives int64
 *   words: workgroups, rows per workgroup, frames per workgroup, LDS bytes per workgroup, row bands, frame pieces; then per workgroup
 *   the rectangle it counts: first row, end row, first frame, end frame.  The grid depends on n, the layout and the range only.
 *   *used = words needed (SP_ERR_INVALID_ARG if capacity is smaller, or 0 <= x_begin <= x_end <= width does not hold).
 * Out of scope: batches, groups and sharding.py (their merge would be an element-wise sum), and a bound on the workspace.
 */
int sp_density_from_index(sp_context *ctx, const uint8_t *d_index, int32_t n, int32_t width, int32_t waterfall, int32_t lut_len,
                          uint32_t *d_density, int32_t accumulate);
int sp_plan_execute_density(sp_plan *plan, const void *d_bytes, size_t nbytes, int32_t width, uint32_t *d_density, int32_t accumulate);
int sp_render_density(sp_context *ctx, const sp_request *req, const uint8_t *bytes, size_t nbytes, int32_t width, uint32_t *density);
int sp_debug_density_launch(int32_t n, int32_t width, int32_t waterfall, int32_t x_begin, int32_t x_end, int64_t *out, size_t capacity,
                            size_t *used);

/*
 * Page-locked host memory for request / reply buffers: sp_render moves pinned buffers at the full rate of the host link, pageable
 * ones through the runtime's staging copies.  The N-API addon backs the reply ArrayBuffers it hands out with these.
 */
int sp_host_alloc(size_t nbytes, void **ptr);
void sp_host_free(void *ptr);
/* Page-locks (and later releases) memory the caller owns, e.g. a reply block that is being recycled. */
int sp_host_register(void *ptr, size_t nbytes);
void sp_host_unregister(void *ptr);

/* Device memory helpers so that non-HIP hosts (Node, ctypes) can keep operands resident. */
int sp_device_alloc(sp_context *ctx, size_t nbytes, void **d_ptr);
int sp_device_free(sp_context *ctx, void *d_ptr);
int sp_device_upload(sp_context *ctx, void *d_dst, const void *src, size_t nbytes);
int sp_device_download(sp_context *ctx, void *dst, const void *d_src, size_t nbytes);
int sp_device_memset(sp_context *ctx, void *d_ptr, int value, size_t nbytes);

/*
 * Benchmark input: fills d_bytes with `count` samples of the seeded tone + noise signal (definition: DESIGN.md,
 * tests/siggen.py 'trinoise'), starting at global sample index t0.  Bit-identical to the CPU generators.
 */
int sp_synth_trinoise(sp_context *ctx, void *d_bytes, int32_t format, uint64_t t0, uint64_t count,
                      uint32_t seed, uint32_t step, uint32_t gshift, double amp, double namp);

/* Elapsed milliseconds of the last sp_plan_execute's main kernel on this context (HIP events on its stream). */
int sp_context_last_kernel_ms(sp_context *ctx, float *ms);
/* Enables (1) / disables (0) per-execute HIP event timing; off by default. */
int sp_context_enable_timing(sp_context *ctx, int32_t on);
/*
 * Calibration for the figure above: elapsed milliseconds of the same event pair around a one-wavefront no-op kernel on the
 * context's stream (minimum of several tries).  It is the dispatch latency an event pair adds to whatever it brackets; a
 * profiler's kernel duration (rocprofv3 --kernel-trace) does not contain it.
 */
int sp_context_event_pair_overhead_ms(sp_context *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif
