/*
 * marex_hip.h -- C ABI of the MI355X (gfx950) hot path behind marEx-style preprocess_data().
 *
 * The reference (wienkers/marEx) is pure Python and has NO plugin / FFI interface: its boundary for
 * this path is the Python call marEx.preprocess_data() (marEx/detect.py:287-313).  This header is
 * therefore the build-defined drop-in boundary: one entry point per numerical stage
 * of that call, each citing the reference lines it replaces.  The Python host side
 * (marex_amd/detect.py) binds it with ctypes; INTEGRATION.md shows the stub a marEx maintainer
 * would add.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error; marex_last_error(ctx) gives the text.
 *  - no exceptions / longjmp cross the ABI; the library owns only the opaque context and the device scratch buffers
 *    inside it (freed by marex_destroy); every data buffer belongs to the caller.
 *  - ALL data pointers are DEVICE pointers (small tables included), except in the entry points suffixed "_h" (the chunk
 *    codec of the Zarr stores), which take HOST pointers.
 *  - work is enqueued on the context's HIP stream (marex_set_stream); marex_sync waits for it.
 *  - field layout is the reference's C-order (time, cells): element (t, c) at [t*C + c].
 *  - one context per (device, host thread).
 */
#ifndef MAREX_HIP_H
#define MAREX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAREX_ABI_VERSION 2
#define MAREX_NDOY 366

typedef struct marex_ctx marex_ctx;

/* statistics of the threshold stage, device resident (detect.py:2707-2732 warnings) */
typedef struct marex_thr_stats {
    uint32_t min_key;   /* order-preserving key of the smallest un-clamped threshold (0xFFFFFFFF if none) */
    uint32_t max_key;   /* order-preserving key of the largest threshold (0 if none)                      */
    uint32_t n_too_low; /* thresholds < lower_bound (they are clamped to it)                              */
    uint32_t n_too_high;/* thresholds > upper_bound                                                       */
    uint32_t n_unresolved; /* outputs a threshold kernel gave up on (written as NaN): an internal error, the host
                              side raises ProcessingError when it is not 0 (never observed; marex_tails.hip, straggler passes) */
    uint32_t reserved[3];
} marex_thr_stats;  /* 32 bytes; callers zero it except min_key = 0xFFFFFFFF */

/* kernel ids for marex_timing_get */
enum {
    MAREX_K_SYNTH = 0,
    MAREX_K_SHIFTING = 1,     /* smoothing + rolling climatology + anomaly + binning + validation */
    MAREX_K_THRESHOLDS = 2,   /* pooled day-of-year histogram quantile                             */
    MAREX_K_MASK = 3,         /* anomaly >= threshold                                              */
    MAREX_K_TRANSPOSE = 4,
    MAREX_K_FIXED = 5,
    MAREX_K_DETREND = 6,
    MAREX_K_EXACT = 7,
    MAREX_K_GLOBAL = 8,
    MAREX_K_STDNORM = 9,      /* day-of-year std, 30-day wrapped rolling RMS, anomaly / STD                 */
    MAREX_K_MORPH = 10,       /* tracker pre-processing: spatial closing + opening, temporal closing       */
    MAREX_K_TAILS = 11,       /* tail extraction (upper end of every dayofyear histogram)                   */
    MAREX_K_COUNT = 12
};

int marex_abi_version(void);

/* Sizes of the caller-owned device buffers of one spatial block (the caller owns every data buffer, the library
 * only its handle and scratch).  bytes[MAREX_WS_COUNT] in the order of the enum; MAREX_WS_TOTAL = what one pass of
 * shifting_baseline / fixed_baseline + hobday_extreme needs beside the input (anomalies, mask bytes, thresholds in both layouts,
 * key lists + aux OR the bin matrix, per-cell mask and counts).  Returns -1 for a null pointer or an impossible shape. */
typedef struct marex_workspace_cfg {
    int64_t T;        /* input timesteps                                                              */
    int64_t T_out;    /* kept timesteps (T minus the first window_year_baseline years for shifting_baseline) */
    int64_t C;        /* cells of the block, overlap rows included                                      */
    int max_bucket;   /* rows of the largest dayofyear bucket                                           */
    int list_rows;    /* rows per key list: 15 (lists emitted by the anomaly kernel), 32 (extraction kernel), 0: bin-matrix path */
} marex_workspace_cfg;
enum {
    MAREX_WS_ANOMALY = 0,   /* float [T_out][C]                         */
    MAREX_WS_EXTREME = 1,   /* uint8 [T_out][C]                         */
    MAREX_WS_THRESHOLDS = 2,/* float [366][C], dayofyear-major AND cell-major: two buffers of this size */
    MAREX_WS_LISTS = 3,     /* key lists [366][NPER][nch][C] x 16 bytes (0 on the bin-matrix path)     */
    MAREX_WS_AUX = 4,       /* uint32 [366][C] (0 on the bin-matrix path)                              */
    MAREX_WS_BINS = 5,      /* uint16 [ceil(C/16)][T_out][16] (0 on the list path)                     */
    MAREX_WS_PER_CELL = 6,  /* uint8 mask [C] + int32 invalid_count [C]                                */
    MAREX_WS_TOTAL = 7,
    MAREX_WS_COUNT = 8
};
int marex_workspace_bytes(const marex_workspace_cfg* cfg, size_t* bytes);
/* A context owns small device scratch buffers that its launches share: use one context per (device, host thread,
 * stream); launches through one context are stream-ordered and must not overlap on different streams. */
int marex_create(int device, marex_ctx** out);
int marex_destroy(marex_ctx* ctx);
const char* marex_last_error(marex_ctx* ctx);
int marex_set_stream(marex_ctx* ctx, void* hip_stream);
int marex_sync(marex_ctx* ctx);

/* Tuning / diagnostic options (tile shapes, forced kernel variants ...; DESIGN.md lists them).  Options live in the context:
 * environment variables MAREX_<NAME>=<int> that exist when the context is created seed the table once, afterwards only
 * these calls change it -- nothing reads the environment at launch time.  name == NULL clears every option. */
int marex_set_option(marex_ctx* ctx, const char* name, int value);
int marex_clear_option(marex_ctx* ctx, const char* name);
/* Event counters of the tail kernels (host uint64[8], synchronises the stream): [0] column rebuilds, [1] probes the per-cell and pooled threshold kernels recounted from every chunk,
 * [2] extra passes for stragglers, [3] days walked (per tile and block),
 * [4] (4-cell, dayofyear) groups the mask kernel decided on the anomalies, [5..7] unused (always 0).
 * The pooled threshold kernel adds per workgroup: [0] one when its first chunks waited in LDS, [2] one, [3] its days.
 * reset != 0 zeroes them afterwards. */
int marex_debug_counters(marex_ctx* ctx, uint64_t* out8, int reset);

/* per-kernel device timing with HIP events on the context's stream (used by bench.py) */
int marex_timing_enable(marex_ctx* ctx, int on);
int marex_timing_reset(marex_ctx* ctx);
int marex_timing_get(marex_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);

/* Synthetic SST field of marex_amd/synth.py, bit-identical to the NumPy version (test/bench utility). */
int marex_synth_sst_f32(marex_ctx* ctx, const float* mean, const float* amp, const uint8_t* hemi,
                        const uint8_t* land, const float* seas /*[T,2]*/, const float* trend /*[T]*/,
                        uint64_t seed, int64_t cell_base, int64_t T, int64_t C, float* x /*[T,C]*/);

/*
 * Shifting-baseline anomaly, fused with validation counting and histogram binning.
 * Replaces: _validate_data_values (detect.py:205-279), smoothed_rolling_climatology (1691-1816),
 * rolling_climatology (1511-1688), _compute_anomaly_shifting_baseline (1819-1850), the year trim
 * (615-641) and the np.digitize step of _compute_histogram_quantile_2d (2622-2631).
 *
 *  year_plan[n_cal_years*366][4]  int32 {timestep, output row, bin-matrix row, 0} of (calendar-year index,
 *                           dayofyear-1); -1 where absent / not an output (rows of the first W years are
 *                           trimmed: detect.py:638-641).  16-byte aligned.  Built on the host from dt.year /
 *                           dt.dayofyear (marex_amd/calendar.py); bin-matrix rows are the kept timesteps sorted
 *                           by (dayofyear, time).
 *  write_clim               0: out = x - clim (anomaly); 1: out = clim (rolling_climatology API)
 *  edges[nb+1], bins        bin table and output bin matrix, uint16, T_out rows (both may be NULL: no binning).
 *                           BIN MATRIX LAYOUT (all entry points): blocks of 16 consecutive cells; element
 *                           (row r, cell c) at ((c >> 4) * T_out + r) * 16 + (c & 15); ceil(C/16)*T_out*16 elements;
 *                           rows are the kept timesteps sorted by (dayofyear, time) (rowb_index)
 *  mask[C]                  isfinite(x[0, c])                     (may be NULL)
 *  invalid_count[C]         number of non-finite x[t, c] over t; must be zeroed by the caller (may be NULL)
 */
int marex_shifting_baseline_f32(marex_ctx* ctx, const float* x, int64_t T, int64_t C,
                                const int32_t* year_plan, int n_cal_years, int W, int S,
                                int write_clim, const float* edges, int nb, int64_t T_out, float* out,
                                uint16_t* bins, uint8_t* mask, int32_t* invalid_count);

/*
 * Day-of-year thresholds from pooled histograms (approximate percentile method).
 * Replaces: the flox 2-D count + spatial pooling + per-cell _rolling_histogram_quantile +
 * NaN-masking + clamp of _compute_histogram_quantile_2d (detect.py:2638-2732, 2465-2559).
 *
 *  bins               uint16 bin matrix in the blocked layout described at marex_shifting_baseline_f32
 *  doy_start[367]     rows doy_start[d-1]..doy_start[d]-1 hold dayofyear d
 *  max_bucket         largest number of rows of one dayofyear (host knows doy_start); lets the kernel use
 *                     16-bit counters when max_bucket*wd*ws*ws <= 65535.  0 = unknown (32-bit counters)
 *  ny, nx             grid (cells = ny*nx, lon fastest); ny == 0: unstructured, no pooling (ws must be <= 1)
 *  first_anom[C]      first kept anomaly row; NaN there => threshold NaN (detect.py:2704)
 *  centres[nb]        float32 bin centres, centres[0] == 0
 *  q, wd, ws          quantile in (0,1], odd day window (3..365), odd spatial window (1 = none)
 *  lower/upper_bound  edges[3] / edges[-2]
 *  row0, row1         gridded only: thresholds are produced for grid rows row0 <= j < row1 (the rows a
 *                     latitude shard owns; its overlap rows only feed the pooling).  Other rows of
 *                     thr_doy_major are left untouched.  Pass 0, ny for everything.
 *  thr_doy_major      out [366, C]   (dayofyear-major working layout used by marex_mask_ge_doy_f32)
 *  stats              device struct, must be initialised {0xFFFFFFFF, 0, 0, 0} by the caller
 */
int marex_hobday_thresholds_f32(marex_ctx* ctx, const uint16_t* bins, int64_t T_out, int64_t C, int ny,
                                int nx, const int32_t* doy_start, int max_bucket, const float* first_anom,
                                const float* centres, int nb, double q, int wd, int ws,
                                float lower_bound, float upper_bound, int row0, int row1,
                                float* thr_doy_major, marex_thr_stats* stats);

/*
 * extreme[t, c] = anom[t, c] >= thr[doy(t), c]   (detect.py:2003-2004) and the count of True (833-835).
 *  doy_rows[T_out]   output rows sorted by (dayofyear, time); doy_start as above
 *  c0, c1            only cells c0 <= c < c1 are compared, written and counted (owned cells of a shard)
 *  n_true            device counter, must be zeroed by the caller (may be NULL)
 */
int marex_mask_ge_doy_f32(marex_ctx* ctx, const float* anom, const float* thr_doy_major,
                          const int32_t* doy_start, const int32_t* doy_rows, int64_t T_out, int64_t C,
                          int64_t c0, int64_t c1, uint8_t* extreme, unsigned long long* n_true);

/* The same mask, read from the bin matrix marex_shifting_baseline_f32 / marex_digitize_f32 produced for these anomalies
 * (`bins`, `edges[0..nb]` as passed there): a sample whose bin lies above / below the bin of its threshold is decided
 * without its value; only samples in the threshold's own bin or in the overflow bin nb are compared as numbers.  Same
 * result bit for bit, 2 instead of 4 bytes read per sample.  Falls back to marex_mask_ge_doy_f32 for shapes its 4-cell
 * kernel does not cover (C, c0, c1 not multiples of 4; unaligned pointers). */
int marex_mask_ge_doy_bins_f32(marex_ctx* ctx, const float* anom, const uint16_t* bins, const float* edges, int nb,
                               const float* thr_doy_major, const int32_t* doy_start, const int32_t* doy_rows, int64_t T_out,
                               int64_t C, int64_t c0, int64_t c1, uint8_t* extreme, unsigned long long* n_true);

/*
 * TAILS: the default representation of the day-of-year histograms of the approximate Hobday method for long series
 * (marEx/detect.py:2622-2648: np.digitize + the flox 2-D count by (dayofyear, bin)).  Only the upper end of a histogram
 * decides a high quantile, so instead of a dense (366 x nb) count per cell the device keeps the samples of every
 * (dayofyear, cell) bucket as 16-bit keys in short lists that are sorted descending; consumers read the top of each list
 * and stop at the first key they do not need:
 *   key = ((bin + 1) << 7) | pos    bin = np.digitize(anom, edges) - 1 (< nb <= 511), pos = index of the sample inside the
 *                                   bucket (output row doy_rows[doy_start[d] + pos], < 128); 0 = empty slot; samples the
 *                                   reference's histogram drops (NaN, >= edges[nb]) have no key
 *   lists  uint16, [366][NPER][NCH][C][8]  chunk j (0: the 8 largest ...) of list p of bucket (d, c).  A bucket's keys are
 *                                   partitioned over NPER = marex_tail_lists(max_bucket, list_rows) = ceil(max_bucket /
 *                                   list_rows) lists of <= list_rows keys, each sorted descending, in NCH = 2 (list_rows
 *                                   <= 16) or 4 (<= 32) chunks of 8 keys.  list_rows = 32: marex_tail_extract_f32 on any
 *                                   anomaly field; list_rows = 15: what marex_shifting_baseline_tails_f32 emits itself
 *   aux    uint32, [366][C]         bits 0..9: number of keys of the bucket (= the samples the reference counts);
 *                                   bit 15: the bucket holds a non-NaN value >= edges[nb] (beyond the table: no key, but an
 *                                   extreme of every finite threshold); bits 16..22 / 23..29: position of the first /
 *                                   second such sample, bit 30: the second exists, bit 31: more than two
 * Rows are grouped by dayofyear through doy_start / doy_rows; max_bucket = rows of the largest dayofyear (<= 128).
 */
int marex_tail_lists(int max_bucket, int list_rows);
int marex_tail_extract_f32(marex_ctx* ctx, const float* anom, int64_t T_out, int64_t C, const int32_t* doy_start,
                           const int32_t* doy_rows, int max_bucket, const float* edges, int nb, int list_rows, void* lists,
                           uint32_t* aux);

/* The shifting-baseline anomaly stage of marex_shifting_baseline_f32 emitting TAILS (list_rows = 15) instead of the bin
 * matrix: the kernel sorts the keys of 15 output years at a time and writes them as one list per dayofyear; dayofyears its
 * fast path does not take (irregular calendars, smoothing / baseline windows without a fast instance) get their lists from
 * the anomalies afterwards -- the lists are complete either way.  -4: nb > 511, max_bucket > 90 or C > 2^24. */
int marex_shifting_baseline_tails_f32(marex_ctx* ctx, const float* x, int64_t T, int64_t C, const int32_t* year_plan,
                                      int n_cal_years, int W, int S, const float* edges, int nb, int64_t T_out, float* out,
                                      uint8_t* mask, int32_t* invalid_count, const int32_t* doy_start, const int32_t* doy_rows,
                                      int max_bucket, void* lists, uint32_t* aux);

/* Day-of-year thresholds from tails: same result as marex_hobday_thresholds_f32 (detect.py:2638-2732, 2465-2559: pooled
 * counts, count-interpolated quantile, NaN where the first kept anomaly is NaN, clamp and warning statistics), arguments as
 * there plus the tails and the anomaly field they belong to (`anom`, [T_out, C]: its row 0 is first_anom).
 * Needs nb <= 511, max_bucket <= 128 in at most 6 lists, ws <= 7, max_bucket*wd*ws*ws <= 65535 and C <= 2^24 (else -4: use
 * the bin-matrix entry point). */
int marex_hobday_thresholds_tails_f32(marex_ctx* ctx, const void* lists, const uint32_t* aux, int list_rows, const float* anom,
                                      int64_t T_out, int64_t C, int ny, int nx, int max_bucket, const float* centres, int nb,
                                      double q, int wd, int ws, float lower_bound, float upper_bound, int row0, int row1,
                                      float* thr_doy_major, marex_thr_stats* stats);

/* Day-of-year thresholds from tails, pooled over mesh neighbour rings (no reference counterpart: the reference does not pool
 * on unstructured meshes).  The histogram of cell c is the sum of the histograms of pool[0..K)[c]: `pool` is int32 [K][C] on the
 * device, member-major, row 0 = the cell itself, -1 = empty slot, no duplicates, K <= 13 (two rings of at most three neighbours).
 * Everything after the sum is marex_hobday_thresholds_tails_f32 with ws = 1: count-interpolated quantile, NaN where the cell's OWN
 * first kept anomaly is NaN, clamp, statistics.  Thresholds are written for the cells [c0, c1) only; members may lie anywhere in
 * [0, C).  The entries of the rows c0..c1 are range-checked on the host before the launch (one device-to-host copy of the table):
 * -1 for an index outside -1..C-1 or a row 0 that is not the cell.  -4: nb > 511, max_bucket > 128, max_bucket*wd*K > 65535 or
 * C > 2^24.  Options: THR_POOL_RING = 1 / 0 (the first chunks of the window's lists wait in LDS / are read from global memory at
 * every probe; default: in LDS whenever the ring fits), THR_POOL_BLOCKS = day blocks per 64 cells.  Same bits on either path. */
int marex_hobday_thresholds_pool_f32(marex_ctx* ctx, const void* lists, const uint32_t* aux, int list_rows, const float* anom,
                                     int64_t T_out, int64_t C, int max_bucket, const int32_t* pool, int K, int64_t c0, int64_t c1,
                                     const float* centres, int nb, double q, int wd, float lower_bound, float upper_bound,
                                     float* thr_doy_major, marex_thr_stats* stats);

/* The extreme mask from tails: same result as marex_mask_ge_doy_f32 (detect.py:2003-2004, 833-835) without reading the
 * anomalies, except for samples in the threshold's own bin and for buckets holding more than two values beyond the edge table
 * (up to two are placed from the positions in aux). */
int marex_mask_ge_doy_tails_f32(marex_ctx* ctx, const void* lists, const uint32_t* aux, int list_rows, int max_bucket,
                                const float* anom, const float* edges, int nb, const float* thr_doy_major,
                                const int32_t* doy_start, const int32_t* doy_rows, int64_t T_out, int64_t C, int64_t c0,
                                int64_t c1, uint8_t* extreme, unsigned long long* n_true);

/*
 * Fixed-baseline anomaly (detect.py:2299-2397): clim[d, c] = float32 nanmean of x over the timesteps with
 * dayofyear d (only those with use_row[t] != 0 when use_row is given: reference_period, 2334-2361),
 * out[t, c] = x[t, c] - clim[doy(t), c] for ALL timesteps.  doy_start / doy_rows describe all T rows
 * (calendar built without trim).  bins / mask / invalid_count as in marex_shifting_baseline_f32
 * (bins rows are the dayofyear-sorted rows; invalid_count must be zeroed by the caller).
 */
int marex_fixed_baseline_f32(marex_ctx* ctx, const float* x, int64_t T, int64_t C, const int32_t* doy_start,
                             const int32_t* doy_rows, const uint8_t* use_row, const float* edges, int nb,
                             float* out, uint16_t* bins, uint8_t* mask, int32_t* invalid_count);
/* The same stage with an optional per-cell value `sub[C]` taken off every sample on load (one float32 subtraction, as
 * detect.py:2222-2224 does for the whole field): folds the last pass of a force_zero_mean detrend into this one.
 * `max_bucket` = rows of the largest dayofyear bucket (0 = unknown): up to 128 rows without a bin matrix the field is read
 * once (buckets held in registers). */
int marex_fixed_baseline_sub_f32(marex_ctx* ctx, const float* x, const float* sub, int max_bucket, int64_t T, int64_t C,
                                 const int32_t* doy_start, const int32_t* doy_rows, const uint8_t* use_row,
                                 const float* edges, int nb, float* out, uint16_t* bins, uint8_t* mask,
                                 int32_t* invalid_count);

/* bins[rowb_index[t], c] = np.digitize(anom[t, c], edges) - 1 for rows with rowb_index[t] >= 0 (detect.py:2622-2631) */
int marex_digitize_f32(marex_ctx* ctx, const float* anom, int64_t T, int64_t C, const int32_t* rowb_index,
                       const float* edges, int nb, int64_t T_out, uint16_t* bins);

/*
 * Polynomial / harmonic detrend (detect.py:2143-2224).  pmodel[T, n_coef] = pinv(model) and
 * model_t[T, n_coef] = model^T, float64, computed on the host (marex_amd/calendar.py:detrend_model).
 * out = x - fl32(model^T (pmodel^T x)), minus its time mean when force_zero_mean.  mask / invalid_count
 * are written (not accumulated) when given.  The two reductions over time are float64 partial sums over blocks of
 * 1024 consecutive timesteps (ascending t) combined in ascending block order -- the order oracle.detrend_anomaly
 * fixes (the reference's BLAS order is unspecified).  Scratch lives in the context.
 */
int marex_detrend_f32(marex_ctx* ctx, const float* x, int64_t T, int64_t C, const double* pmodel,
                      const double* model_t, int n_coef, int force_zero_mean, float* out, uint8_t* mask,
                      int32_t* invalid_count);
/* detect.py:2143-2224 with force_zero_mean, the mean NOT yet subtracted: `out` = residuals, `mean[C]` = fl32(sum / T)
 * (the value marex_detrend_f32 would subtract); for callers that subtract while reading (marex_fixed_baseline_sub_f32). */
int marex_detrend_deferred_mean_f32(marex_ctx* ctx, const float* x, int64_t T, int64_t C, const double* pmodel,
                                    const double* model_t, int n_coef, float* out, float* mean, uint8_t* mask,
                                    int32_t* invalid_count);
/* detect.py:2400-2462 (detrend_fixed_baseline) as one chain: fit, residual mean, and the daily climatology stage recomputing
 * the residuals from x while it reads (3 reads and 1 write of the field; the residual field is never materialised).
 * n_coef <= 5 and max_bucket <= 128, else -4 (run marex_detrend_deferred_mean_f32 + marex_fixed_baseline_sub_f32 instead).
 * model_sorted[r][k] = model_t[doy_rows[r]][k]: the model rows in dayofyear-sorted row order (contiguous per bucket).
 * mask / invalid_count: of the RAW field, as marex_detrend_f32 reports them. */
int marex_detrend_fixed_baseline_f32(marex_ctx* ctx, const float* x, int64_t T, int64_t C, const double* pmodel,
                                     const double* model_t, const double* model_sorted, int n_coef, int force_zero_mean,
                                     const int32_t* doy_start,
                                     const int32_t* doy_rows, const uint8_t* use_row, int max_bucket, float* out,
                                     uint8_t* mask, int32_t* invalid_count);
/* The two fixed-baseline stages above (detect.py:2299-2397, 2400-2462) that also leave the sorted key lists of their own output
 * -- exactly what marex_tail_extract_f32(out, list_rows = 32) would write (TAILS, below): `lists` [366][NPER][4][C] x 16 bytes with
 * NPER = marex_tail_lists(max_bucket, 32), `aux` [366][C]; the bucket is in registers when its anomalies are formed, so the
 * threshold stage needs no extraction pass (a read of the whole anomaly field: 13 ms per 100-yr band, round 3).  `edges[0..nb]`
 * as for marex_tail_extract_f32; nb <= 511, max_bucket <= 128 (-4 otherwise: run the plain entry point + marex_tail_extract_f32). */
int marex_fixed_baseline_tails_f32(marex_ctx* ctx, const float* x, const float* sub, int max_bucket, int64_t T, int64_t C,
                                   const int32_t* doy_start, const int32_t* doy_rows, const uint8_t* use_row,
                                   const float* edges, int nb, float* out, uint8_t* mask, int32_t* invalid_count,
                                   void* lists, uint32_t* aux);
int marex_detrend_fixed_baseline_tails_f32(marex_ctx* ctx, const float* x, int64_t T, int64_t C, const double* pmodel,
                                           const double* model_t, const double* model_sorted, int n_coef,
                                           int force_zero_mean, const int32_t* doy_start, const int32_t* doy_rows,
                                           const uint8_t* use_row, int max_bucket, const float* edges, int nb, float* out,
                                           uint8_t* mask, int32_t* invalid_count, void* lists, uint32_t* aux);

/*
 * Exact Hobday percentile (detect.py:1921-1956): thr[d, c] = np.nanpercentile(anom[doy in window(d), c], p),
 * float32, NumPy 2.x "linear" rule, no spatial pooling; output layout [366, C] (= the reference's
 * (dayofyear, space) order for this method).  q32 = float32(p) / float32(100) computed by the caller with
 * NumPy; max_window_rows = largest number of rows in any wd-day window; *overflow (device int, zeroed by
 * the caller) counts cells whose selection buffer was too small (must stay 0).
 */
int marex_hobday_exact_f32(marex_ctx* ctx, const float* anom, int64_t T_out, int64_t C, const int32_t* doy_start,
                           const int32_t* doy_rows, int max_window_rows, float q32, double q, int wd,
                           float* thr_doy_major, int32_t* overflow);

/*
 * Global (constant-in-time) threshold per cell (detect.py:2873-2912).
 *  exact != 0 : float64 np.nanquantile(anom[:, c], q) ("linear"), edges/centres/stats/minmax unused.
 *  exact == 0 : _compute_histogram_quantile_1d (2737-2865) on float64 edges[nb+1] / centres[nb]; thresholds
 *               below lower_bound are clamped; stats counts the out-of-range thresholds and minmax[2]
 *               (device, initialised {+inf, -inf}) receives the un-clamped extremes for the warning text.
 */
int marex_global_threshold_f32(marex_ctx* ctx, const float* anom, int64_t T_out, int64_t C, double q, int exact,
                               const double* edges, const double* centres, int nb, double lower_bound,
                               double upper_bound, double* thr, marex_thr_stats* stats, double* minmax);

/* Validation verdict (marEx/detect.py:205-279, `_validate_data_values`) from what the anomaly entry points leave per cell
 * (`mask` = isfinite(x[0]), `invalid_count` = non-finite values over time), over cells c0 .. c1-1 (a shard's owned cells):
 * out4 (device int64[4]) = {ocean cells, invalid values in ocean cells, ocean cells affected, worst cell's count} --
 * the numbers of the reference's two error messages; shards combine them with one all-reduce (sum, sum, sum, max). */
int marex_validation_summary(marex_ctx* ctx, const uint8_t* mask, const int32_t* invalid_count, int64_t c0, int64_t c1,
                             int64_t* out4);

/* extreme[t, c] = anom[t, c] >= thr[c] (comparison in float64, detect.py:2915) and the count of True */
int marex_mask_ge_const_f32(marex_ctx* ctx, const float* anom, const double* thr, int64_t T_out, int64_t C,
                            uint8_t* extreme, unsigned long long* n_true);

/* std_normalise branch of detrend_harmonic, part 1 (marEx/detect.py:2257-2273):
 *   std_day[d, c]  = population standard deviation (ddof = 0) of anom[t, c] over the rows with dayofyear d + 1 --
 *                    NaN when a term is NaN or the dayofyear never occurs; float64 two-pass (mean, then squared
 *                    deviations, both summed in ascending time), one float64 sqrt, rounded to float32
 *   std_roll[d, c] = float32 sqrt of the centred `window`-day mean of float32(std_day^2) on the wrapped dayofyear
 *                    axis (offsets -window/2 .. window-1-window/2; float64 sum in ascending offset, / window,
 *                    rounded to float32; NaN when a term is NaN)  -- the reference's `STD` variable (window = 30).
 * doy_start / doy_rows: rows of `anom` grouped by dayofyear (int32 [367] / [T]).  std_day is caller workspace. */
int marex_std_rolling_doy_f32(marex_ctx* ctx, const float* anom, int64_t T, int64_t C, const int32_t* doy_start,
                              const int32_t* doy_rows, int window, float* std_day, float* std_roll);

/* part 2 (detect.py:2275-2278): out[t, c] = anom[t, c] / (std_roll[doy(t), c] > 1e-10 ? std_roll : NaN), float32 division */
int marex_div_doy_f32(marex_ctx* ctx, const float* anom, const float* std_roll, const int32_t* doy_start,
                      const int32_t* doy_rows, int64_t T, int64_t C, float* out);

/* Tracker pre-processing, gridded data (marEx/track.py:1520-1676): per timestep, pad the binary image by 2 R cells on
 * every side (regional_mode 0: np.pad "wrap" in both dimensions, 1: "edge"), binary closing then binary opening with the
 * disk x^2 + y^2 < R^2 + 1 (scipy.ndimage semantics, border_value 0), trim the padding, AND with the ocean mask.
 * data / out: uint8 [T, ny, nx] (0 / 1); mask: uint8 [ny, nx].  R = 0: only the mask is applied.  R in 0..63.  No pointer
 * needs more than byte alignment (the 8-byte stores are taken for nx % 8 == 0 with mask and out 8-byte aligned only). */
int marex_fill_holes_u8(marex_ctx* ctx, const uint8_t* data, const uint8_t* mask, int64_t T, int ny, int nx, int R,
                        int regional_mode, uint8_t* out);

/* Temporal binary closing with T_fill + 1 consecutive steps (T_fill even), False outside the series
 * (track.py:1694-1721); the caller follows it with marex_fill_holes_u8(R / 2) as the reference does (1724). */
int marex_time_closing_u8(marex_ctx* ctx, const uint8_t* data, int64_t T, int64_t C, int T_fill, uint8_t* out);

/* Connected components of every timestep on its own (track.py:2013-2031 with time_connectivity = False): 8-connected in
 * (y, x), periodic in x when wrap_x.  labels[i] = 1 + smallest linear index (into the whole [T, ny, nx] array) of the
 * component of cell i, 0 = background -- unique across time like the reference's IDs, but numbered differently from
 * scipy's scan order; areas[r] = number of cells of the component whose smallest index is r, 0 elsewhere. */
int marex_label2d_i32(marex_ctx* ctx, const uint8_t* data, int64_t T, int ny, int nx, int wrap_x, int32_t* labels,
                      int32_t* areas);

/* Connected components in (time, y, x) (track.py:2006-2048, structured grid, time_connectivity = True): 26-connected,
 * periodic in x when wrap_x; connect_t = 0 drops the links to t-1 (time_connectivity = False, one labelling per step).
 * ids[i] = 1 + rank of the component's first cell in C order among all components (IDs 1..N, scipy.ndimage.label's
 * scan order, which the reference's dask_image labelling keeps), 0 = background; areas[id - 1] = cells of component id
 * (capacity: T * ny * nx entries, the first N written); *n_out = N.  Fewer than 2^31 - 1 cells. */
int marex_label3d_i32(marex_ctx* ctx, const uint8_t* data, int64_t T, int ny, int nx, int wrap_x, int connect_t, int32_t* ids,
                      int32_t* areas, int32_t* n_out);

/* Labelling in time blocks, for fields of 2^31 - 1 cells and more (marex_label3d_i32 takes fewer): the caller labels
 * contiguous blocks of timesteps with marex_label3d_i32 into the slices of one ids[T][ny * nx], block k giving local IDs
 * 1..n_k; its provisional global IDs are off_k + local, off_k = n_0 + ... + n_{k-1}, N_prov = the sum (at most 2^31 - 2).
 * table: int32 [table_len = N_prov + 1], table[g] = g on entry (entry 0 = background) -- a parent array over the
 * provisional IDs.
 *
 * marex_label_seam_union_i32: one seam.  prev_ids = the last slice of block k, next_ids = the first slice of block k+1
 *   (int32 [ny * nx] each, still local IDs); every cell of next_ids unions its ID with those of its up to nine
 *   neighbours in prev_ids (3 x 3 in (y, x), x periodic when wrap_x), the larger root hooked under the smaller.
 *   Not called with connect_t = 0.  IDs outside 1..n_prev / 1..n_next are ignored.
 * marex_label_table_resolve_i32: after all seams.  table[g] becomes the final ID of provisional ID g: 1 + the number of
 *   roots (smallest provisional ID of an event) below g's root, table[0] = 0 -- the numbering of one labelling call over
 *   the whole field.  prov_areas: int32 [n_prov], cells of provisional ID g at g - 1 (the blocks' areas, concatenated);
 *   areas: int64 [n_prov], areas[id - 1] = cells of final ID id, the first *n_out entries meaningful; *n_out = N.
 * marex_label_apply_table_i32: ids[i] = ids[i] > 0 ? table[off + ids[i]] : 0 in place over the n cells of one block
 *   (off = off_k; n < 2^31 - 1).
 * All three are asynchronous on the context's stream. */
int marex_label_seam_union_i32(marex_ctx* ctx, const int32_t* prev_ids, const int32_t* next_ids, int ny, int nx, int wrap_x,
                               int off_prev, int n_prev, int off_next, int n_next, int32_t* table, int64_t table_len);
int marex_label_table_resolve_i32(marex_ctx* ctx, int32_t* table, int64_t n_prov, const int32_t* prov_areas, int64_t* areas,
                                  int32_t* n_out);
int marex_label_apply_table_i32(marex_ctx* ctx, int32_t* ids, int64_t n, const int32_t* table, int64_t table_len, int off);

/* out[i] = labels[i] > 0 && labels[i] != drop_label && areas[labels[i] - 1] >= area_threshold (track.py:1891-1903;
 * drop_label = the reference's `object_ids_keep[0] = -1`, which removes the first object of the list) */
int marex_filter_by_area_u8(marex_ctx* ctx, const int32_t* labels, const int32_t* areas, int64_t n,
                            double area_threshold, int drop_label, uint8_t* out);

/* Ordered stream compaction: the positive entries of v[0..n) (n <= 2^31 - 2), in index order, to out[0..cap) -- the
 * per-object areas that marex_label2d_i32 / marex_label_mesh_i32 leave at the root cells, as a list ordered by (time,
 * first cell).  *n_out (device) = their number, *first_index (device) = the index of the first one, -1 when there is none.
 * Synchronises the stream once to learn the count: with more than cap positive entries the first cap are written,
 * *n_out still holds the full count and the call returns -7.  Separate launches (tile counts, scan, scatter): no
 * workgroup waits on another. */
int marex_compact_positive_i32(marex_ctx* ctx, const int32_t* v, int64_t n, int32_t* out, int64_t cap, int64_t* n_out,
                               int64_t* first_index);

/* The same two stages on an unstructured mesh (track.py:1543-1606 and 1932-2004): nbr int32 [3, C], 0-based, -1 = no
 * neighbour (the reference's `neighbours - 1`).  fill_holes: dilation by R = R sweeps of "OR over the cell and its listed
 * neighbours"; closing with the land set True before the erosion, then opening, NO final land mask (as in the reference).
 * label: components over the listed edges (undirected), land excluded; labels / areas as in marex_label2d_i32. */
int marex_fill_holes_mesh_u8(marex_ctx* ctx, const uint8_t* data, const uint8_t* mask, const int32_t* nbr, int64_t T,
                             int64_t C, int R, uint8_t* out);
int marex_label_mesh_i32(marex_ctx* ctx, const uint8_t* data, const uint8_t* mask, const int32_t* nbr, int64_t T, int64_t C,
                         int32_t* labels, int32_t* areas);

/* Host-side (the only entry point taking HOST pointers, hence "_h"): decode one Blosc-1 frame -- LZ4 codec or memcpy,
 * byte shuffle or none -- the chunk format of the reference's Zarr v2 stores ({"id": "blosc", "cname": "lz4",
 * "shuffle": 1}; examples/batch jobs/run_detect.py:55-83, the fixtures under tests/data).  0 = OK and *out_len = decoded bytes;
 * -5 malformed frame, -6 unsupported codec / filter. */
int marex_blosc_decompress_h(const void* src, int64_t srclen, void* dst, int64_t dstcap, int64_t* out_len);
/* Zstandard frames (RFC 8878, no dictionaries; the content checksum is skipped), host pointers: the inner codec of the Blosc
 * frames of the small coordinate arrays in the reference's stores ({"cname": "zstd"}; xr.open_zarr, run_detect.py:55).
 * Returns 0 and the decoded length, -5 for a malformed / unsupported stream, never reads or writes out of bounds. */
int marex_zstd_decompress_h(const uint8_t* src, int64_t srclen, uint8_t* dst, int64_t dstcap, int64_t* out_len);

/* Host-side inverse: compress nbytes bytes into one Blosc-1 frame (LZ4 codec; byte shuffle when shuffle != 0 and
 * typesize > 1; blocksize <= 0 = 256 KiB) -- the chunk format `extremes_ds.to_zarr(...)` produces through numcodecs'
 * default compressor (examples/batch jobs/run_detect.py:83).  Blocks are split into `typesize` streams exactly when every
 * c-blosc 1.x decoder expects it; incompressible streams / frames are stored, so dstcap >= nbytes + 16 always suffices.
 * 0 = OK and *out_len = frame bytes; -1 bad argument, -4 destination too small. */
int marex_blosc_compress_h(const void* src, int64_t nbytes, int typesize, int shuffle, int64_t blocksize, void* dst,
                           int64_t dstcap, int64_t* out_len);

/* Device-side inverse of marex_blosc_compress_h (the chunk format of `extremes_ds.to_zarr(...)`, examples/batch
 * jobs/run_detect.py:83, for arrays held in HBM): n_chunks chunks of nbytes bytes, chunk i at src + i * nbytes (device),
 * become frames byte-identical to marex_blosc_compress_h(chunk i, nbytes, typesize, shuffle, blocksize, dst, nbytes + 16,
 * ...): frame i at dst + i * (nbytes + 16) (device), its length in out_len[i] (device int64).  work: device scratch of
 * marex_blosc_compress_work_bytes(nbytes, typesize, shuffle, blocksize, n_chunks) bytes.  variant 0 encodes every LZ4
 * stream with one wave (speculative hashing of 64 positions), 1 with one lane (the serial loop); both write the same bytes.
 * Asynchronous on the context's stream. */
int marex_blosc_compress_work_bytes(int64_t nbytes, int typesize, int shuffle, int64_t blocksize, int64_t n_chunks,
                                    int64_t* out);
int marex_blosc_compress_d(marex_ctx* ctx, const uint8_t* src, int64_t nbytes, int64_t n_chunks, int typesize, int shuffle,
                           int64_t blocksize, int variant, uint8_t* work, int64_t work_bytes, uint8_t* dst, int64_t* out_len);

/* Device-side chunk decoding (compressed bytes cross PCIe, the field is born in HBM): n_streams LZ4 block streams --
 * stream s = comp[src_off[s] .. +csize[s]) -> planes[dst_off[s] .. +rawsz[s]) (csize == rawsz: stored, copied) -- one
 * wave each; *status (device int, zeroed by the caller) counts malformed streams.  Then marex_unshuffle_place turns the
 * byte planes of every Blosc block (planes + blk_off[b], blk_ne[b] elements of `typesize` bytes, byte-shuffled or not)
 * into elements blk_elem0[b] .. +blk_valid[b] of the destination array `out`.  The host parses the frame headers
 * (marex_amd/zarr_io.py). */
int marex_lz4_decode_streams(marex_ctx* ctx, const uint8_t* comp, const int64_t* src_off, const int32_t* csize,
                             const int64_t* dst_off, const int32_t* rawsz, int n_streams, int max_raw, uint8_t* planes,
                             int32_t* status);
int marex_unshuffle_place(marex_ctx* ctx, const uint8_t* planes, const int64_t* blk_off, const int64_t* blk_elem0,
                          const int32_t* blk_ne, const int32_t* blk_valid, int n_blocks, int max_ne, int typesize, int shuffled,
                          uint8_t* out);

/* Object properties and time overlaps of an int32 ID field ids[T][C] (C = ny * nx; values <= 0 are background; C and T
 * below 2^31 - 1).  Used by tracker.calculate_object_properties / find_overlapping_objects (marEx/track.py:2109-2504).
 *
 * marex_ids_minmax_i32: minmax[0] = min, minmax[1] = max of ids[0 .. n).
 * marex_object_spans_i32: tmin[id] / tmax[id] = first / last timestep with a cell of id (INT_MAX / -1 when absent), for
 *   id = 0 .. max_id (max_id >= every ID); off[id] = exclusive prefix sum in ID order of the spans tmax - tmin + 1, so that
 *   slot off[id] + t - tmin[id] belongs to (t, id); *total = the number of slots.  work: int64 [2 * ceil((max_id + 1) / 4096)].
 * marex_object_moments_i32: acc[slot][0..4] = cell count, sum of y, sum of x, cells with x > nx / 2, flags (bit 0: a cell
 *   with x < 100, bit 1: a cell with x >= nx - 100) of every slot; acc [n_slots][5] is zeroed first.  Integer atomics
 *   only: bitwise reproducible.
 * marex_object_compact: the slots with a non-zero count -> out_tid[p] = (t, id), out_mom[p][0..4] = acc[slot], in no
 *   particular order; *n_out = how many.  out_tid [n_slots][2], out_mom [n_slots][5].
 * marex_overlap_count_i32: over the cells of slices t < T - 1, stats[0] = cells with ids[t] > 0 and ids[t + 1] > 0,
 *   stats[1] = the runs of equal (ids[t], ids[t + 1]) pairs the device folds together (>= the distinct pairs);
 *   stats[2], stats[3] = 0.
 * marex_overlap_pairs_i32: the distinct pairs and their cell counts.  keys / counts: a table of cap (a power of two,
 *   >= 2 * stats[1] recommended) u64 entries each, zeroed here; out_keys[p] = id_t << 32 | id_t+1, out_counts[p] = cells,
 *   p < stats[3], in no particular order (at most out_cap written); stats[2] != 0 when the table overflowed. */
int marex_ids_minmax_i32(marex_ctx* ctx, const int32_t* ids, int64_t n, int32_t* minmax);
int marex_object_spans_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, int max_id, int32_t* tmin, int32_t* tmax,
                           int64_t* off, int64_t* work, int64_t* total);
int marex_object_moments_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int ny, int nx, const int32_t* tmin,
                             const int64_t* off, int64_t n_slots, uint64_t* acc);
int marex_object_compact(marex_ctx* ctx, int64_t n_slots, int max_id, const int32_t* tmin, const int64_t* off,
                         const uint64_t* acc, uint64_t* n_out, int32_t* out_tid, uint64_t* out_mom);
int marex_overlap_count_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, uint64_t* stats);
int marex_overlap_pairs_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, int64_t cap, uint64_t* keys,
                            uint64_t* counts, uint64_t* stats, int64_t out_cap, uint64_t* out_keys, uint64_t* out_counts);

/* The same object stages on an unstructured mesh (marEx/track.py:1947-2005, 2135-2323, 2431-2439, 1513-1514, 2762-2764),
 * area weighted in fixed point.  q: int64 [4][C], row-major: q[0][c] = rint(area * 2^e), q[1..3][c] = rint(area * x, y, z
 * * 2^e) with (x, y, z) the unit vector of cell c; the host picks e so that |sum over c of any row| < 2^62
 * (marex_amd.track.mesh_weight_tables).  The device adds these integers with 64-bit integer atomics only: results are
 * bitwise reproducible and independent of the launch shape.  ids: int32 [T][C], values <= 0 are background; C and T
 * below 2^31 - 1.
 *
 * marex_label_mesh_rank_i32: labels [T][C] of marex_label_mesh_i32 (1 + smallest linear index of the component in this
 *   [T][C] block, T * C < 2^31 - 1) -> ids[t][c] = the rank of the cell's component among the components of timestep t
 *   by smallest cell index, 1 .. n_t[t] (scipy.sparse.csgraph.connected_components order, track.py:1979-1982), 0 for
 *   background; n_t: int32 [T].  rank: int32 [T * C] work (only root cells are written and read; the areas array of
 *   marex_label_mesh_i32 may be given).  ids may be labels (in place).
 * marex_ids_row_max_i32: rowmax[t] = max(0, max over c of ids[t][c]), int32 [T].
 * marex_ids_add_row_offset_i32: out[t][c] = ids[t][c] > 0 ? ids[t][c] + off[t] : 0 (off: int32 [T]; the caller makes sure
 *   the sums fit int32); out may be ids.  Together: the IDs made unique in time of track.py:2762-2764.
 * marex_mesh_object_moments_i64: slots as in marex_object_spans_i32; acc[slot][0] = cells, acc[slot][1..4] = sums of
 *   q[0..3][c] over the cells of the slot (two's complement); acc [n_slots][5] is zeroed first; marex_object_compact
 *   lists the non-empty slots.
 * marex_mesh_overlap_pairs_i64: marex_overlap_pairs_i32 with the sum of q0[c] (= q[0]) over the cells of the pair in
 *   place of their number; marex_overlap_count_i32 sizes the table (stats as there).  A pair met in many timesteps can
 *   exceed 64 bits, so a sum is two words: sums [cap][2] and out_sums [out_cap][2], the pair's sum = word 1 * 2^32 + word 0
 *   (word 0 collects the low 32 bits of the partial sums and may itself exceed 2^32).
 * marex_mesh_area_i64: out[t] = sum over c of data[t][c] != 0 ? q0[c] : 0, data uint8 [T][C]; out uint64 [T], zeroed
 *   first.
 * marex_mesh_event_rename_i64 (cluster_rename_objects_and_props on a mesh: the apply_ufunc map, process_timestep and
 *   calculate_area_centroid_for_slice, track.py:2908-2926, 2948-2989, 3161-3210, in one pass): in place, ids[t][c] = ev =
 *   lut[v] for 0 < v = ids[t][c] < lut_len, else 0; an ev outside 1 .. n_ev counts as background too.  For ev > 0 the
 *   dense slot s = t * n_ev + ev - 1 takes acc[s][0..4] += 1, q[0..3][c] and gid[s] = max(gid[s], v): the largest
 *   original ID under the slot.  lut: int32 [lut_len]; acc [T * n_ev][5] and gid int32 [T * n_ev] are zeroed first.
 *   -1 for a null pointer or an empty shape, -4 for C or T of 2^31 - 1 or more.
 * All are asynchronous on the context's stream. */
int marex_label_mesh_rank_i32(marex_ctx* ctx, const int32_t* labels, int64_t T, int64_t C, int32_t* rank, int32_t* ids,
                              int32_t* n_t);
int marex_ids_row_max_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, int32_t* rowmax);
int marex_ids_add_row_offset_i32(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, const int32_t* off, int32_t* out);
int marex_mesh_object_moments_i64(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, const int64_t* q,
                                  const int32_t* tmin, const int64_t* off, int64_t n_slots, uint64_t* acc);
int marex_mesh_overlap_pairs_i64(marex_ctx* ctx, const int32_t* ids, int64_t T, int64_t C, const int64_t* q0, int64_t cap,
                                 uint64_t* keys, uint64_t* sums, uint64_t* stats, int64_t out_cap, uint64_t* out_keys,
                                 uint64_t* out_sums);
int marex_mesh_area_i64(marex_ctx* ctx, const uint8_t* data, int64_t T, int64_t C, const int64_t* q0, uint64_t* out);
int marex_mesh_event_rename_i64(marex_ctx* ctx, int32_t* ids, int64_t T, int64_t C, const int32_t* lut, int64_t lut_len,
                                int n_ev, const int64_t* q, uint64_t* acc, int32_t* gid);

/* Stages of the merge tracker on grids (tracker.split_and_merge_objects / consolidate_object_ids /
 * cluster_rename_objects_and_props, marEx/track.py:2554-3802).  Slices are int32 [ny][nx], fields int32 [T][ny][nx];
 * values <= 0 are background.  Distances are float64 sqrt(dy * dy + dx * dx), dx wrapped by +-nx when |dx| > nx / 2 and
 * wrap != 0; the first nearest parent wins.
 *
 * marex_relabel_i32 (replaces the `where(data != child, first)` renames of track.py:2629-2631 and the apply_ufunc map of
 *   2897-2924): ids[i] = vals[j] where keys[j] == ids[i] (keys ascending, distinct; IDs without an entry unchanged) or,
 *   with keys == NULL, ids[i] = vals[ids[i]] for 0 < ids[i] < n_keys.  In place.
 * marex_partition_centroid_i32 (wrapped_euclidian_distance_mask_parallel + argmin, track.py:3548-3553, 4826-4873): every
 *   cell of child child_keys[k] (ascending) takes lab[j] of the parent entry j in off[k] .. off[k + 1] whose centroid
 *   (pcy[j], pcx[j]) is nearest.  In place, all merging children of one iteration at once.
 * marex_nn_bucket_count_i32 / marex_partition_nn_i32 (partition_nn_grid, track.py:4972-5113): parent entry j has bucket
 *   size gs[j], ngy[j] x ngx[j] buckets at base[j] .. of n_buckets, search radius maxd[j]; parent ID par_keys[q]
 *   (ascending) owns entries pent[poff[q] .. poff[q + 1]).  The count pass sets bstart[0 .. n_buckets] to the exclusive
 *   scan of the (cell of prev, entry) counts per bucket (cnt: work, n_buckets); bstart[n_buckets] = n_cells.  The
 *   partition pass sorts those cells into cells[n_cells] by bucket (cursor: work, n_buckets) and gives every child cell
 *   of ids the label of the parent with the nearest cell in the 3 x 3 buckets around its own (bucket indices periodic in
 *   y and x) within maxd, else of the nearest centroid.
 * marex_event_moments_i32 (calculate_area_centroid_for_slice and process_timestep, track.py:2936-2976, 3140-3247): for
 *   slot s = t * n_ev + e - 1 of the event field ev (1 .. n_ev): acc[s][0..4] = cells, sum y, sum x, sum of
 *   (x > nx / 2 ? x - nx : x), flags (1: a cell with x < 100, 2: a cell with x >= nx - 100); gid[s] = the largest ID of
 *   orig under the slot's cells (0 when empty); with w (float32 [ny][nx]) also wacc[s][0..3] = float64 sums of w, w y,
 *   w x, w x_shifted.  acc, gid (and wacc) are zeroed first; integer sums are bitwise reproducible.
 * marex_event_rename_i32 (the apply_ufunc map of track.py:2897-2924 and the pass above fused, in place, with compact
 *   slots): ids int32 [T][ny * nx]; e = lut[v] for 0 < v = ids[t][c] < lut_len, else 0, an e outside 1 .. n_ev becomes 0,
 *   and e is written back where it differs from v.  Event e owns the slots ev_off[e] .. ev_off[e + 1] - 1, one per
 *   timestep from ev_tmin[e] on (ev_tmin int32 [n_ev + 1], ev_off int64 [n_ev + 2], entry 0 unused / 0; n_slots =
 *   ev_off[n_ev + 1]): a cell of e at t goes to s = ev_off[e] + t - ev_tmin[e].  acc uint64 [n_slots][5], gid int32
 *   [n_slots] (the largest v under the slot) and, with w, wacc float64 [n_slots][4] as in marex_event_moments_i32; all
 *   three and status are zeroed first.  A cell whose event lies outside its declared span (t < ev_tmin[e] or
 *   s >= ev_off[e + 1], or s >= n_slots) is renamed but not accumulated and adds one to status[0] (uint64 [1]): no slot
 *   index that was not range-checked addresses acc, gid or wacc.  -1: null pointer or empty shape; -4: ny * nx or T of
 *   2^31 - 1 or more (the field itself may hold any number of cells: it is addressed with 64-bit offsets). */
int marex_relabel_i32(marex_ctx* ctx, int32_t* ids, int64_t n, const int32_t* keys, const int32_t* vals, int n_keys);
int marex_partition_centroid_i32(marex_ctx* ctx, int32_t* ids, int ny, int nx, const int32_t* child_keys, int n_child,
                                 const int32_t* off, const double* pcy, const double* pcx, const int32_t* lab, int wrap);
int marex_nn_bucket_count_i32(marex_ctx* ctx, const int32_t* prev, int ny, int nx, const int32_t* par_keys, int n_par,
                              const int32_t* poff, const int32_t* pent, const int32_t* gs, const int32_t* ngy,
                              const int32_t* ngx, const int64_t* base, int64_t n_buckets, int64_t* cnt, int64_t* bstart);
int marex_partition_nn_i32(marex_ctx* ctx, int32_t* ids, const int32_t* prev, int ny, int nx, const int32_t* par_keys,
                           int n_par, const int32_t* poff, const int32_t* pent, const int32_t* child_keys, int n_child,
                           const int32_t* off, const double* pcy, const double* pcx, const int32_t* lab, const int32_t* gs,
                           const int32_t* ngy, const int32_t* ngx, const int32_t* maxd, const int64_t* base,
                           int64_t n_buckets, const int64_t* bstart, int64_t* cursor, int32_t* cells, int64_t n_cells,
                           int wrap);
int marex_event_moments_i32(marex_ctx* ctx, const int32_t* ev, const int32_t* orig, int64_t T, int ny, int nx, int n_ev,
                            const float* w, uint64_t* acc, double* wacc, int32_t* gid);
int marex_event_rename_i32(marex_ctx* ctx, int32_t* ids, int64_t T, int ny, int nx, const int32_t* lut, int64_t lut_len,
                           int n_ev, const int32_t* ev_tmin, const int64_t* ev_off, int64_t n_slots, const float* w,
                           uint64_t* acc, double* wacc, int32_t* gid, uint64_t* status);

/* Per-(timestep, event) intensity of tracked events: the event field joined with the anomaly field it was detected in (the
 * reference leaves this to notebook code, groupby / where over ID_field and dat_anomaly).
 *
 * marex_event_intensity_f32: ids int32 [Tb][C] and anom float32 [Tb][C] are the rows t0 .. t0 + Tb - 1 of the field (a grid
 *   slice flattened, or a mesh); values of ids outside 1 .. n_ev are background.  The slots are those of
 *   marex_event_rename_i32: event e owns ev_off[e] .. ev_off[e + 1] - 1, one per timestep from ev_tmin[e] on (ev_tmin int32
 *   [n_ev + 1], ev_off int64 [n_ev + 2], entry 0 unused / 0), and a cell of e in row r goes to s = ev_off[e] + (t0 + r) -
 *   ev_tmin[e].  w: float32 [C] cell weights, or NULL for unit weights.  A cell with a finite anomaly a adds cnt[s][0] += 1,
 *   sums[s][0] += (double)w, sums[s][1] += (double)w * (double)a (an exact product) and vmax[s] = max(vmax[s], key(a)),
 *   key the order-preserving map of a float32 to uint32 (b = the bits of a; key = b | 2^31 for b < 2^31, ~b otherwise):
 *   key 0 belongs to no finite value and means "no finite cell".  A cell whose anomaly is NaN or +-inf adds cnt[s][1] += 1
 *   and nothing else.  cnt uint64 [n_slots][2], sums float64 [n_slots][2], vmax uint32 [n_slots], status uint64 [1]: the
 *   function only adds -- the caller zeroes all four before the first block, so a field is walked in time blocks into the
 *   same slots.  A cell whose event lies outside its declared span (t < ev_tmin[e], s >= ev_off[e + 1] or s >= n_slots)
 *   adds one to status[0] and nothing else: no slot index that was not range-checked addresses cnt, sums or vmax.  The
 *   anomalies (and weights) are fetched only under cells of an event.
 *   Arithmetic: the counts and the maximum are exact and independent of any order.  The float64 sums are atomic adds of
 *   exact terms: bit for bit reproducible whenever the partial sums are exactly representable, otherwise within
 *   2 n u sum|w a| of the exact sum (n the finite cells of the slot, u = 2^-53; the order-independent bound of recursive
 *   summation) -- the precedent of the weighted moments wacc of marex_event_rename_i32, not the integer contract of the
 *   mesh areas.
 *   -1: null pointer, empty shape, t0 < 0, n_ev <= 0 or n_slots <= 0; -4: C or t0 + Tb of 2^31 - 1 or more (the field itself
 *   may hold any number of cells: it is addressed with 64-bit offsets).  Asynchronous on the context's stream. */
int marex_event_intensity_f32(marex_ctx* ctx, const int32_t* ids, const float* anom, int64_t t0, int64_t Tb, int64_t C,
                              int n_ev, const int32_t* ev_tmin, const int64_t* ev_off, int64_t n_slots, const float* w,
                              uint64_t* cnt, double* sums, uint32_t* vmax, uint64_t* status);

/* Shape of tracked events on a grid: per (timestep, event) the integer sums behind extent, perimeter, axes and centroid paths
 * (the reference hands such properties to regionprops_table; the side-count perimeter and the orientation convention are
 * this project's own).
 *
 * marex_event_shapes_i32: ids int32 [Tb][ny * nx] are the rows t0 .. t0 + Tb - 1 of a gridded field, cell (y, x) at y * nx + x;
 *   values outside 1 .. n_ev are background.  n_ev, ev_tmin, ev_off, n_slots and the slot s of a cell as in
 *   marex_event_intensity_f32.  regional != 0: the columns left of 0 and right of nx - 1 are domain border; otherwise x is
 *   periodic (with nx = 1 a cell is its own east and west neighbour).  The rows above 0 and below ny - 1 are always border.
 *   A side of an event cell is exposed when the neighbour across it holds a different value (0 included) or lies outside the
 *   domain; each of the four sides is tested on its own.
 *   mom uint64 [n_slots][16], per cell of the slot:
 *     0 cells   1 sum y   2 sum x   3 cells with x > nx / 2   4 flags, OR-ed (1: a cell with x < 100, 2: one with x >= nx - 100)
 *     5 sum y^2   6 sum x^2   7 sum x y   8 sum x over the cells with x > nx / 2   9 sum y over them
 *     10 exposed sides facing north or south   11 facing east or west   12 exposed sides on the domain border
 *     13 exposed sides whose neighbour is inside the domain and 0 in mask (uint8 [ny * nx], or NULL: none)
 *     14 sum of the lengths of the exposed sides: ns_q[y] for a north side, ns_q[y + 1] for a south side, ew_q[y] for an
 *        east or west side (ns_q int64 [ny + 1] and ew_q int64 [ny], given together, or both NULL: 0)
 *     15 sum of area_q[y * nx + x] (int64 [ny * nx], or NULL: 0)
 *   box int32 [n_slots][6]: min y, max y, min x and max x over the cells with x <= nx / 2, min x and max x over those with
 *   x > nx / 2 (atomic minima and maxima; the caller fills the minima with INT_MAX and the maxima with -1 first).
 *   status uint64 [1].  The function only accumulates: the caller prepares mom (zero), box and status before the first block,
 *   so a field is walked in time blocks into the same slots; the stencil stays inside a slice, so blocks need no halo.  A cell
 *   whose event lies outside its declared span adds one to status[0] and nothing else: no slot index that was not
 *   range-checked addresses mom or box.  The four neighbours, the mask bytes and the table rows are fetched only under cells
 *   of an event.  Every sum is an integer: exact, and independent of any order and of the blocks.
 *   Bounds: with ny, nx <= 65536 and a slice below 2^31 cells, sum x^2 <= nx^2 n < 2^63 (sum y^2 likewise) and sum x y <
 *   2^62; the caller scales the tables so that no sum of them reaches 2^62.
 *   -1: null pointer, empty shape, t0 < 0, n_ev <= 0, n_slots <= 0, or ns_q / ew_q given in part; -4: ny or nx above 65536, or
 *   ny * nx or t0 + Tb of 2^31 - 1 or more.  Asynchronous on the context's stream. */
int marex_event_shapes_i32(marex_ctx* ctx, const int32_t* ids, int64_t t0, int64_t Tb, int ny, int nx, int regional, int n_ev,
                           const int32_t* ev_tmin, const int64_t* ev_off, int64_t n_slots, const uint8_t* mask,
                           const int64_t* area_q, const int64_t* ns_q, const int64_t* ew_q, uint64_t* mom, int32_t* box,
                           uint64_t* status);

/* Shape of tracked events on an unstructured mesh of three-sided cells: per (timestep, event) the integer sums behind
 * perimeter, coastal contact, axes on the sphere and centroid paths (this project's own definitions; the reference has
 * nothing of the kind).
 *
 * marex_mesh_event_shapes_i64: ids int32 [Tb][C] are the rows t0 .. t0 + Tb - 1 of a mesh field; values outside 1 .. n_ev are
 *   background.  n_ev, ev_tmin, ev_off, n_slots and the slot s of a cell as in marex_event_intensity_f32.  nbr int32 [3][C]:
 *   the cell across the k-th side of cell c, 0-based; a value outside 0 .. C - 1 (-1 by convention) is "no neighbour" and is
 *   never used as an index.  A side k of an event cell c with j = nbr[k][c] is exposed when there is no neighbour (then it is
 *   also a border side) or when ids[j] of the same row differs from the cell's value as it stands (0 and numbers above n_ev
 *   included); each of the three slots is tested on its own, so a neighbour listed twice counts twice.
 *   mom uint64 [n_slots][16], per cell of the slot:
 *     0 cells   1 .. 10 the sums of q[0][c] .. q[9][c] (q int64 [10][C]; rows 1 .. 9 are signed, the sums two's complement)
 *     11 exposed sides   12 exposed sides without a neighbour (border)
 *     13 exposed sides whose neighbour exists and is 0 in mask (uint8 [C], or NULL: none)
 *     14 sum of len_q[k][c] over the exposed sides (int64 [3][C], or NULL: 0)
 *     15 exposed sides whose neighbour holds a value above 0 (contact with another event)
 *   box int32 [n_slots][6]: min and max of lat_k[c]; min and max of lon_k[c] over the cells with lon_k[c] < 0; min and max of
 *   lon_k[c] over the cells with lon_k[c] >= 0 (lat_k, lon_k int32 [C], together or both NULL: box is left alone; atomic
 *   minima and maxima; the caller fills the minima with INT_MAX and the maxima with INT_MIN first).
 *   status uint64 [1].  The function only accumulates: the caller prepares mom (zero), box and status before the first block,
 *   so a field is walked in time blocks into the same slots; the neighbours stay inside a row, so blocks need no halo.  A cell
 *   whose event lies outside its declared span adds one to status[0] and nothing else: no slot index that was not
 *   range-checked addresses mom or box.  The neighbours, the mask bytes, the table rows, the lengths and the keys are fetched
 *   only under cells of an event.  Every sum is an integer: exact, and independent of any order and of the blocks.
 *   Bounds: the caller scales q so that the sum of any row over any set of cells stays below 2^62 in magnitude, and len_q so
 *   that the sum over any set of its entries does.
 *   -1: null pointer, empty shape, t0 < 0, n_ev <= 0, n_slots <= 0, or lat_k / lon_k given in part; -4: C or t0 + Tb of
 *   2^31 - 1 or more.  Asynchronous on the context's stream. */
int marex_mesh_event_shapes_i64(marex_ctx* ctx, const int32_t* ids, int64_t t0, int64_t Tb, int64_t C, int n_ev,
                                const int32_t* ev_tmin, const int64_t* ev_off, int64_t n_slots, const int32_t* nbr,
                                const uint8_t* mask, const int64_t* q, const int64_t* len_q, const int32_t* lat_k,
                                const int32_t* lon_k, uint64_t* mom, int32_t* box, uint64_t* status);

/* Severity categories of tracked events (Hobday et al. 2018: moderate, strong, severe, extreme as multiples of the
 * threshold): the event field joined with the anomaly field and the day-of-year thresholds, per (timestep, event).
 *
 * marex_event_categories_f32: ids, anom, t0, Tb, C, n_ev, ev_tmin, ev_off and n_slots as in marex_event_intensity_f32 (the
 *   same slots s = ev_off[e] + t - ev_tmin[e]).  thr float32 [n_doy][C]; doy int32 [T], indexed by the global step t = t0 +
 *   row, gives the row of thr of every step and must reach t0 + Tb.  w: float32 [C] cell weights with cat_area, or both
 *   NULL.  A cell of an event with a finite anomaly a has, with h = thr[doy[t]][c] and the float32 products h2 = 2 h, h3 =
 *   3 h, h4 = 4 h (one rounding each), the class k of marex_local_intensity_*: 5 where h is NaN, +-inf or <= 0, else 0 for
 *   a < h, 1 for h <= a < h2, 2 for h2 <= a < h3, 3 for h3 <= a < h4, 4 for a >= h4.  A cell whose anomaly is NaN or +-inf
 *   has class 6: counted, not classified.
 *   cat_cnt uint64 [n_slots][7]: cat_cnt[s][k] += 1 per cell.  cat_area float64 [n_slots][6]: cat_area[s][k] += (double)w[c]
 *   for k = 0 .. 5, under the summation contract of sums of marex_event_intensity_f32 (exact terms, atomic adds).
 *   field uint8, or NULL: the base of the WHOLE [T][C] output, addressed with the global step as the mask of
 *   marex_cell_events_u8 is.  Every cell of the rows t0 .. t0 + Tb - 1 is written: 0 where the cell belongs to no event,
 *   k + 1 otherwise (7: a non-finite anomaly).  No atomic touches field.
 *   status uint64 [2].  A cell whose event lies outside its declared span (t < ev_tmin[e], s >= ev_off[e + 1] or s >=
 *   n_slots) adds one to status[0] and nothing else, and gets 0 in field: no slot index that was not range-checked
 *   addresses cat_cnt or cat_area.  Under a row whose doy label lies outside 0 .. n_doy - 1 nothing in thr is addressed:
 *   its event cells add one each to status[1] and nothing else, and the row of field is 0.
 *   anom is fetched only under cells of an event, thr and w only under those of them with a finite anomaly.  The function
 *   only adds: the caller zeroes cat_cnt, cat_area and status before the first block.  The counts and field are exact and
 *   independent of any order and of the blocks.
 *   -1: the conditions of marex_event_intensity_f32 (cat_cnt for cnt), thr or doy NULL, n_doy <= 0, or w and cat_area given
 *   in part; -4: as marex_event_intensity_f32.  Asynchronous on the context's stream. */
int marex_event_categories_f32(marex_ctx* ctx, const int32_t* ids, const float* anom, int64_t t0, int64_t Tb, int64_t C,
                               int n_ev, const int32_t* ev_tmin, const int64_t* ev_off, int64_t n_slots, const float* thr,
                               const int32_t* doy, int n_doy, const float* w, uint64_t* cat_cnt, double* cat_area,
                               uint8_t* field, uint64_t* status);

/* Occurrence statistics of an event mask (extreme_events) or a tracked ID field, from one streaming pass (the reference
 * leaves them to notebook code: 03_visualise_events over ID_field, 01_preprocess_extremes over extreme_events).
 *
 * marex_occurrence_u8 / marex_occurrence_i32: x uint8 / int32 [Tb][C] are the rows t0 .. t0 + Tb - 1 of the field (a grid
 *   slice flattened, or a mesh).  A cell is present when x > 0 (match == 0) or when x == match (match > 0).  A negative
 *   int32 cell is never present and adds one to status[0].
 *   cell_cnt uint32 [G][C]: cell_cnt[grp[t]][c] += 1 per present row -- (ID_field > 0).mean("time") with G = 1,
 *   .groupby("time.season").mean("time") with season labels, (ID_field == id).sum("time") with match = id; the caller
 *   divides.  grp int32 [T] is indexed by the global step t = t0 + row and must reach t0 + Tb; NULL with G == 1: every
 *   step is group 0.  A label outside 0 .. G - 1 addresses nothing: its present cells add to status[1].
 *   run_state uint32 [3][C], or NULL: per cell the length of the run of present rows that is open after the rows seen so
 *   far, the number of runs begun, and the longest run.  It is read at the start and written at the end of a call, so a
 *   field walked in any sequence of time windows gives the arrays of one call.
 *   sec_cnt uint64 [G2][R] with sgrp int32 [T] and cls int32 [C], or all three NULL: sec_cnt[sgrp[t]][cls[c]] += 1 per
 *   present cell -- (ID_field > 0).mean("lon").resample(time="ME").mean() with cls = the grid row and sgrp = the month of
 *   the series, .groupby("time.dayofyear").mean(), groupby_bins(lat, bins).mean("ncells") with cls = the latitude bin of
 *   a mesh cell.  A cell whose class lies outside 0 .. R - 1 is counted nowhere; a label of sgrp outside 0 .. G2 - 1
 *   addresses nothing, the present cells with a class add to status[1].  G2 may be as large as T.
 *   status uint64 [2].  The functions only add: the caller zeroes cell_cnt, run_state, sec_cnt and status before the
 *   first window.  All results are integers, exact and independent of the order of execution and of the windows.
 *   The uint8 function reads four cells per lane through 32-bit loads when C % 4 == 0, x is 4-byte and cell_cnt and
 *   run_state are 16-byte aligned, one cell per lane otherwise: same results.
 *   -1: null x, cell_cnt or status, empty shape, t0 < 0, match < 0, G <= 0, NULL grp with G != 1, sec_cnt / sgrp / cls
 *   given in part or with G2 <= 0 or R <= 0; -4: C or t0 + Tb of 2^31 - 1 or more (the field itself may hold any number
 *   of cells: it is addressed with 64-bit offsets).  Asynchronous on the context's stream. */
int marex_occurrence_u8(marex_ctx* ctx, const uint8_t* x, int64_t t0, int64_t Tb, int64_t C, int match, const int32_t* grp,
                        int G, const int32_t* sgrp, int G2, const int32_t* cls, int R, uint32_t* run_state,
                        uint32_t* cell_cnt, uint64_t* sec_cnt, uint64_t* status);
int marex_occurrence_i32(marex_ctx* ctx, const int32_t* x, int64_t t0, int64_t Tb, int64_t C, int match, const int32_t* grp,
                         int G, const int32_t* sgrp, int G2, const int32_t* cls, int R, uint32_t* run_state,
                         uint32_t* cell_cnt, uint64_t* sec_cnt, uint64_t* status);

/* Per-cell intensity of extremes and their severity categories, from one streaming pass over a presence field, the anomaly
 * field and, optionally, the day-of-year thresholds (the reference leaves them to notebook code:
 * dat_anomaly.where(extreme_events).groupby("time.year") sum / mean / max / idxmax; the categories of Hobday et al. 2018 as
 * multiples of the threshold).
 *
 * marex_local_intensity_u8 / marex_local_intensity_i32: x uint8 / int32 [Tb][C] and anom float32 [Tb][C] are the rows
 *   t0 .. t0 + Tb - 1 of the fields.  A cell is present when x > 0 (match == 0) or when x == match (match > 0); a negative
 *   int32 cell is never present and adds one to status[0].  anom and thr are fetched only under present cells.
 *   grp int32 [T] (indexed by the global step, must reach t0 + Tb; NULL with G == 1: every step is group 0) selects the
 *   accumulators of a step, all [G][C]:
 *     days uint32: present steps with a finite anomaly;  invalid uint32: present steps whose anomaly is NaN or +-inf (they
 *     add nothing else);  sum float64: the sequential sum of (double)a over the steps counted in days, in ascending time;
 *     vmax uint32: the largest key(a) (the key of marex_event_intensity_f32; 0: none);  tmax int32: the earliest global
 *     step that attains it (replaced only by a strictly larger key; meaningless where vmax is 0).
 *   Summation contract: within a call, when the first row or a change of the group label begins a stretch, the owning lane
 *   loads sum[g][c], adds one term per step and stores it when the stretch ends; no partial sum is ever added to memory.
 *   sum[g][c] is therefore one fixed sequence of float64 additions: bit-identical to a row-by-row loop, equal from run
 *   to run and independent of how the rows are cut into calls, also for groups that are revisited (seasons, months).
 *   thr float32 [n_doy][C] with doy int32 [T] (the row of thr of every global step) and cat_days uint32 [G][6][C], or all
 *   three NULL: with h = thr[doy[t]][c] and the float32 products h2 = 2 h, h3 = 3 h, h4 = 4 h (one rounding each) a step
 *   counted in days adds one to cat_days[g][k][c], k = 5 where h is NaN, +-inf or <= 0, else 0 for a < h (present below
 *   the threshold: a gap-filled day of a tracked event), 1 for h <= a < h2, 2 for h2 <= a < h3, 3 for h3 <= a < h4, 4 for
 *   a >= h4.
 *   sec_cnt uint64 [G2][R][6] with sgrp int32 [T] and cls int32 [C], or all three NULL (they need thr):
 *   sec_cnt[sgrp[t]][cls[c]][k] += 1 per step classified k.  A cell whose class lies outside 0 .. R - 1 is counted nowhere.
 *   A step whose grp or doy label lies outside 0 .. G - 1 / 0 .. n_doy - 1 addresses nothing: its present cells add to
 *   status[1] and to nothing else; under a label of sgrp outside 0 .. G2 - 1 the classified cells with a class add to
 *   status[1] instead of sec_cnt.  status uint64 [2].
 *   The functions only continue the accumulators: the caller zeroes all of them before the first window.  Everything but
 *   sum is an integer or a maximum: exact and independent of any order.  No atomic touches a per-cell output.
 *   The uint8 function without thr reads four cells per lane through 32-bit loads when C % 4 == 0 and x is 4-byte aligned,
 *   one cell per lane otherwise and with thr: same results.
 *   -1: null x, anom, days, invalid, sum, vmax, tmax or status, empty shape, t0 < 0, match < 0, G <= 0, NULL grp with
 *   G != 1, thr / doy / cat_days given in part or with n_doy <= 0, sec_cnt / sgrp / cls given in part, with G2 <= 0 or
 *   R <= 0, or without thr; -4: C or t0 + Tb of 2^31 - 1 or more (the fields themselves may hold any number of cells: they
 *   are addressed with 64-bit offsets).  Asynchronous on the context's stream. */
int marex_local_intensity_u8(marex_ctx* ctx, const uint8_t* x, const float* anom, int64_t t0, int64_t Tb, int64_t C, int match,
                             const int32_t* grp, int G, const float* thr, const int32_t* doy, int n_doy, const int32_t* sgrp,
                             int G2, const int32_t* cls, int R, uint32_t* days, uint32_t* invalid, double* sum, uint32_t* vmax,
                             int32_t* tmax, uint32_t* cat_days, uint64_t* sec_cnt, uint64_t* status);
int marex_local_intensity_i32(marex_ctx* ctx, const int32_t* x, const float* anom, int64_t t0, int64_t Tb, int64_t C, int match,
                              const int32_t* grp, int G, const float* thr, const int32_t* doy, int n_doy, const int32_t* sgrp,
                              int G2, const int32_t* cls, int R, uint32_t* days, uint32_t* invalid, double* sum, uint32_t* vmax,
                              int32_t* tmax, uint32_t* cat_days, uint64_t* sec_cnt, uint64_t* status);

/* Per-cell events under the duration and gap rule of Hobday et al. (2016), from one streaming pass over an event mask and,
 * optionally, the anomaly field.  Per cell a run of at least min_duration consecutive present steps qualifies (a shorter
 * run is ignored and bridges nothing); walking the qualifying runs in time order, a run that starts at most max_gap steps
 * after the end of the current event extends it, any other run starts a new one.  An event spans start .. end inclusive,
 * gaps included; a run at either end of the record counts by its observed length.
 *
 * marex_cell_events_u8: x uint8 [Tb][C] (present where x > 0) and anom float32 [Tb][C] (or NULL) are the rows
 *   t0 .. t0 + Tb - 1 of the fields.  The state of every cell is carried between calls in state_i32 int32 [4][C] (without
 *   anom) or [10][C] (run length, start + 1 of the open event, its last qualifying step, records written; the event's
 *   maximum key, its step and invalid steps; the same three of the tail) and state_f64 float64 [2][C] (the event's and the
 *   tail's sum; NULL without anom): one plane per variable, zeroed by the caller before the first window.  finish != 0 on
 *   the last window closes the open events at their last qualifying step.
 *   An event that closes adds to the accumulators of the group of its START step, grp[start] (grp int32 [T], global steps,
 *   must reach t0 + Tb; NULL with G == 1), all [G][C] and all NULL or all given: events uint32 += 1, event_days uint32 +=
 *   end - start + 1, duration_max uint32 = max, and with anom sum float64 += the event's sum, vmax uint32 = max of the
 *   event's maximum as an ordered key (0: none), invalid uint32 += the event's non-finite steps.  The intensity of an event
 *   is taken over all steps start .. end.  Its sum has one fixed order: the steps of a run up to the one that qualifies it,
 *   and the steps since the event's last qualifying step before them when the run joins an open event, are summed in
 *   ascending time on their own (the tail) and join the event's sum as one term; every later step of the run is added to
 *   the event's sum directly.  No window boundary changes a bit of it.  anom is fetched only under present steps and
 *   under absent steps of an open event.  A start label outside 0 .. G - 1 addresses nothing: status[0] += 1.
 *   mask uint8 (or NULL) is the base of the WHOLE [T][C] output, addressed with the global step: row t gets 1 where the
 *   cell is in a qualified run, and when a run qualifies the steps of its event not marked yet -- from the run's start, or
 *   from the step after the event's previous end -- are set to 1, also in rows of earlier windows.
 *   rec_off int64 [C + 1] with rec_start and rec_end int32 [n] (and with anom rec_vmax uint32, rec_tmax int32, rec_sum
 *   float64, rec_invalid uint32 [n]), or all NULL: the k-th event that closes in cell c is written at rec_off[c] + k, k
 *   carried in the state; an event past rec_off[c + 1] is not written: status[1] += 1.  status uint64 [2].
 *   Without anom four cells per lane through 32-bit accesses when C % 4 == 0 and x and mask are 4-byte aligned; one cell
 *   per lane otherwise and with anom: same results.  No atomic touches a per-cell output.  Tb == 0 does nothing.
 *   -1: null x, state_i32 or status, anom without state_f64, C <= 0, t0 < 0, Tb < 0, min_duration < 1, max_gap < 0, G <= 0,
 *   NULL grp with G != 1, accumulators or records given in part or their anomaly members without anom, a pointer not
 *   aligned to its element; -4: C or t0 + Tb of 2^31 - 1 or more.  Nothing is launched then.  Asynchronous on the context's
 *   stream. */
int marex_cell_events_u8(marex_ctx* ctx, const uint8_t* x, const float* anom, int64_t t0, int64_t Tb, int64_t C,
                         int min_duration, int max_gap, int finish, const int32_t* grp, int G, int32_t* state_i32,
                         double* state_f64, uint32_t* events, uint32_t* event_days, uint32_t* duration_max, double* sum,
                         uint32_t* vmax, uint32_t* invalid, uint8_t* mask, const int64_t* rec_off, int32_t* rec_start,
                         int32_t* rec_end, uint32_t* rec_vmax, int32_t* rec_tmax, double* rec_sum, uint32_t* rec_invalid,
                         uint64_t* status);

/* Accumulated heat stress of a raw SST field x against a fixed per-cell threshold: the Degree Heating Week of NOAA Coral
 * Reef Watch (Liu et al. 2014, Skirving et al. 2020) -- the monthly mean climatology whose maximum is the threshold m (the
 * MMM), the HotSpot x - m counted from hotspot_min on, its running sum over `window` steps, the bleaching alert class of
 * every step and the maxima per time group.  A lane owns a cell; nothing looks at a neighbour.
 *
 * marex_group_mean_f32: x float32 [Tb][C] are the rows t0 .. t0 + Tb - 1 of the field, lab int32 [T] (indexed by the global
 *   step, must reach t0 + Tb) the label of every step: -1 skips the step, 0 .. G - 1 selects sum float64 [G][C] and cnt
 *   uint32 [G][C]: cnt += 1 and sum += (double)x per finite sample.  Summation contract (that of marex_local_intensity_*):
 *   the owning lane loads sum[g][c] when the first row or a change of the label begins a stretch, adds one term per step
 *   and stores it when the stretch ends; no partial sum is ever added to memory.  sum[g][c] is therefore one sequence of
 *   float64 additions in ascending step: the bits of a row-by-row loop, whatever the windows, also for labels that return.
 *   Under a label outside -1 .. G - 1 a step addresses nothing: each of its C cells adds one to status uint64 [1].
 *   The function only continues sum and cnt: the caller zeroes them before the first window.
 *   -1: null pointer, empty shape, t0 < 0, G <= 0; -4: C or t0 + Tb of 2^31 - 1 or more.
 *
 * marex_heat_stress_f32: x points at row t0 - lead of the field, lead = min(window, t0) rows of history in front of the Tb
 *   rows t0 .. t0 + Tb - 1 of the call; mmm float32 [C] is m.  Per step, with the float32 difference d = x[t] - m (one
 *   rounding): the step is valid when x[t] and m are finite and |d| < 1024; h[t] = d where the step is valid and
 *   d >= hotspot_min, else 0; S[t] = sum of h[k] over k = max(0, t - window + 1) .. t; dhw[t] = float32(S[t] /
 *   steps_per_week), one float64 division and one rounding, NaN in every step of a cell whose m is not finite.
 *   S is carried between calls in state float64 [C], zeroed by the caller before the first window, and updated as
 *   S += h[t]; S -= h[t - window], the leaving step recomputed from x[t - window] and m by the same rule.  That is exact:
 *   1 <= window <= 366 and 2^-10 <= hotspot_min < 1024 make every counted h a multiple of 2^-33 below 2^10, so any sum of
 *   up to 512 of them is a float64; S[t] is the exact real sum whatever the order or the windows.
 *   The alert class of a step, from d, hotspot_min and dhw[t] compared as float32 with levels float32 [L], 0 <= L <= 6,
 *   ascending: 255 where the step is not valid, 0 for d <= 0, 1 for 0 < d < hotspot_min, else 2 + #{j : dhw[t] >= levels[j]}.
 *   grp int32 [T] (global steps, must reach t0 + Tb; NULL with G == 1: every step is group 0) selects the accumulators of
 *   a step, all given or all NULL: dhw_max uint32 [G][C], the largest ordered key (that of marex_event_intensity_f32; 0:
 *   none) of dhw[t] over the steps of a cell with m; tmax int32 [G][C], the earliest global step that attains it
 *   (meaningless where dhw_max is 0); hotspot_max uint32 [G][C], the largest key of d over the valid steps; alert_steps
 *   uint32 [G][3 + L][C], the steps per alert class; invalid uint32 [G][C], the steps that are not valid; onset int32
 *   [G][max(L, 1)][C] (addressed [g][j][c] with L rows per group), ONE PLUS the first global step of the group with
 *   dhw[t] >= levels[j], 0: none.  The caller zeroes them; the lane loads them when a stretch begins and stores them when
 *   it ends, as above.  Under a label outside 0 .. G - 1 a step addresses no accumulator: each of its C cells adds one to
 *   status uint64 [1]; S and the field outputs do not depend on the labels.
 *   dhw float32 and alert uint8 (each may be NULL) are the bases of the WHOLE [T][C] outputs, addressed with the global
 *   step: the rows t0 .. t0 + Tb - 1 are written.  No atomic touches a per-cell output.  One cell per lane.
 *   -1: null x, mmm, state or status, empty shape, t0 < 0, window outside 1 .. 366, lead != min(window, t0), hotspot_min
 *   outside [2^-10, 1024), steps_per_week not positive and finite, L outside 0 .. 6, NULL levels with L > 0, G <= 0, NULL
 *   grp with G != 1, accumulators given in part; -4: C or t0 + Tb of 2^31 - 1 or more (the fields are addressed with
 *   64-bit offsets).  Nothing is launched then.  Both functions are asynchronous on the context's stream. */
int marex_group_mean_f32(marex_ctx* ctx, const float* x, int64_t t0, int64_t Tb, int64_t C, const int32_t* lab, int G,
                         double* sum, uint32_t* cnt, uint64_t* status);
int marex_heat_stress_f32(marex_ctx* ctx, const float* x, const float* mmm, int64_t t0, int64_t lead, int64_t Tb, int64_t C,
                          int window, float hotspot_min, double steps_per_week, const float* levels, int L,
                          const int32_t* grp, int G, double* state, uint32_t* dhw_max, int32_t* tmax, uint32_t* hotspot_max,
                          uint32_t* alert_steps, uint32_t* invalid, int32_t* onset, float* dhw, uint8_t* alert,
                          uint64_t* status);

/* Nearest-cell resampling between two geometries on the sphere: the exact nearest source cell of every target, and the gather
 * of a [time, cells] field through such an index.  Vectors are float64 unit vectors laid out [3][N] (x row, y row, z row);
 * the host computes them, the device calls no transcendental.  The squared chord of a source and a target is
 * q = (dx * dx + dy * dy) + dz * dz, dx = xs - xt etc., each operation rounded on its own; the answer of a target is the
 * source that is smallest in the order (q, cell number): independent of search structure, bucket order, lane and wave.
 *
 * marex_nearest_brute_f64: src [3][N] with the cell numbers ids int32 [N] (NULL: 0 .. N - 1), dst [3][M].  Without sel
 *   (K == M) every target is searched; with sel int32 [K], 1 <= K <= M, only the targets it lists (an entry outside
 *   0 .. M - 1 addresses nothing).  index int32 [M] and q float64 [M] of a searched target receive the winner and its q,
 *   those of the other targets are left as they are.  A target with a NaN
 *   coordinate, or without a source, gets index -1 and q = +inf.
 * marex_voxel_count_f64: count int32 [n^3] (zeroed by the caller) += the sources per voxel of the n^3 grid of edge 2 / n over
 *   [-1, 1]^3; the voxel of a point is (vz * n + vy) * n + vx with v = clamp(int((p + 1) * (n / 2)), 0, n - 1) per axis.
 * marex_voxel_scatter_f64: off int32 [n^3 + 1] is the exclusive prefix sum of count, cursor int32 [n^3] zeroed by the caller;
 *   writes sorted [3][N] and sorted_ids [N], the vectors and cell numbers in voxel order (the order inside a voxel is not
 *   determined).  A position outside 0 .. N - 1 (an offset table of other sources) is not written.
 * marex_nearest_voxel_f64: one target per lane searches the Chebyshev rings r = 0 .. max_rings of voxels around its own.  It
 *   stops after ring r >= 1 when its best q < ((r h)^2) * (1 - 2^-32), h = 2 / n (marex_nearest.hip derives the margin: n <= 1024),
 *   when that bound exceeds qmax (q above qmax is of no interest to the caller; +inf: no limit), or when the rings cover
 *   the grid: flag uint8 [M] = 0 and index / q are final.  A target still open after max_rings gets flag 1 and the best pair
 *   so far: the caller searches it again with marex_nearest_brute_f64.  NaN targets: index -1, q +inf, flag 0.
 * marex_resample_nearest_u8 / _i32 / _f32: out [Tb][M] = x [Tb][C] at index int32 [M]; fill where index < 0 (an index of C
 *   or more reads nothing and gives fill too).  64-bit offsets: Tb * C and Tb * M are not bounded, C and M stay below 2^31 - 1.
 *   No atomics; every element of out is written exactly once.
 *   -1: null pointer, empty shape, K or n or max_rings or qmax or fill (u8: 0 .. 255) out of range; -4: 2^31 - 1 or more
 *   cells or rows.  Nothing is launched then.  All are asynchronous on the context's stream. */
int marex_nearest_brute_f64(marex_ctx* ctx, const double* src, const int32_t* ids, int64_t N, const double* dst, int64_t M,
                            const int32_t* sel, int64_t K, int32_t* index, double* q);
int marex_voxel_count_f64(marex_ctx* ctx, const double* src, int64_t N, int n, int32_t* count);
int marex_voxel_scatter_f64(marex_ctx* ctx, const double* src, const int32_t* ids, int64_t N, int n, const int32_t* off,
                            int32_t* cursor, double* sorted, int32_t* sorted_ids);
int marex_nearest_voxel_f64(marex_ctx* ctx, const double* sorted, const int32_t* sorted_ids, int64_t N, const int32_t* off, int n,
                            const double* dst, int64_t M, int max_rings, double qmax, int32_t* index, double* q, uint8_t* flag);
int marex_resample_nearest_u8(marex_ctx* ctx, const uint8_t* x, int64_t Tb, int64_t C, const int32_t* index, int64_t M, int fill,
                              uint8_t* out);
int marex_resample_nearest_i32(marex_ctx* ctx, const int32_t* x, int64_t Tb, int64_t C, const int32_t* index, int64_t M, int fill,
                               int32_t* out);
int marex_resample_nearest_f32(marex_ctx* ctx, const float* x, int64_t Tb, int64_t C, const int32_t* index, int64_t M, float fill,
                               float* out);

/* Compound events of two presence fields A and B, from one streaming pass over both (the reference's guide builds the
 * joint mask on the host, docs/user_guide.rst:821-833: sst_extremes.extreme_events & salinity_extremes.extreme_events, and
 * leaves every statistic of it to the user).
 *
 * marex_compound_u8: a, b uint8 [Tb][C] are the rows t0 .. t0 + Tb - 1 of the fields; a cell is present where the byte is
 *   not 0.  With A[t], B[t] the presence of a cell at the global step t, L = max_lag and K = tolerance (both 0 .. 30):
 *   cell_cnt uint32 [3][G][C]: per present row cell_cnt[0][grp[t]][c] += A, [1] += B, [2] += A and B.  grp int32 [T] is
 *   indexed by the global step and must reach t0 + Tb; NULL with G == 1: every step is group 0.  A label outside
 *   0 .. G - 1 addresses nothing: the present cells of A and those of B add to status[1].
 *   state uint32 [13][C]: what a cell carries between calls, read at the start and written at the end of a call, so a
 *   record walked in any sequence of time windows gives the arrays of one call.  Rows 0 .. 2: the joint run open after the
 *   rows seen so far, the joint runs begun, the longest joint run (run_state of marex_occurrence_* on A and B).  Rows 3, 4:
 *   the history of A and of B, bit l the presence l steps ago (with L == 0 kept up to bit K; with L > 0 rows 11, 12 hold
 *   the steps 32 .. 61 ago; max_lag and tolerance must be those of the record's first call).  Rows 5, 6: the run coincidence
 *   of A and of B (bit 30: a run is open, bit 31: it has met the other field, bits 0 .. K - 1: unmet runs that ended
 *   i + 1 steps ago).  Rows 7 .. 10: the runs of A, those of them that are coincident, the runs of B, those of them that
 *   are coincident.  A run [s, e] of A (maximal, consecutive present steps) is coincident when B is present at some step
 *   of [max(0, s - K), min(T - 1, e + K)]; the same for B with the roles swapped.  A run open after the last row is a
 *   run, judged on the rows seen.
 *   lag_cnt uint32 [2 L + 1][C], given exactly with L > 0: lag_cnt[L + l][c] is the number of steps t with A[t] and
 *   B[t + l], both steps inside the record, l = -L .. L; row L equals the sum over the groups of cell_cnt[2].
 *   sec_cnt uint64 [3][G2][R] with sgrp int32 [T] and cls int32 [C], or all three NULL: the three counts per (step label,
 *   cell class) as sec_cnt of marex_occurrence_*; under a label outside 0 .. G2 - 1 the cells of A and those of B that
 *   have a class add to status[1].
 *   mask uint8, or NULL: the base of the WHOLE [T][C] joint mask, addressed with the global step.  Every byte of the rows
 *   t0 .. t0 + Tb - 1 is written: 1 where A and B, else 0.  mask must not overlap a or b.
 *   status uint64 [2]; [0] is not used.  The function only continues state, cell_cnt, lag_cnt, sec_cnt and status: the
 *   caller zeroes them before the first window.  All results are integers, exact and independent of the order of
 *   execution and of the windows.  No atomic touches a per-cell output.
 *   Four cells per lane through 32-bit accesses when C % 4 == 0, a, b and mask are 4-byte and state, cell_cnt and lag_cnt
 *   are 16-byte aligned; one cell per lane otherwise: same results.
 *   -1: null a, b, state, cell_cnt or status, empty shape, t0 < 0, G <= 0, NULL grp with G != 1, max_lag or tolerance
 *   outside 0 .. 30, lag_cnt given without max_lag > 0 or missing with it, sec_cnt / sgrp / cls given in part or with
 *   G2 <= 0 or R <= 0; -4: C or t0 + Tb of 2^31 - 1 or more (the fields themselves may hold any number of cells: they are
 *   addressed with 64-bit offsets).  Asynchronous on the context's stream. */
int marex_compound_u8(marex_ctx* ctx, const uint8_t* a, const uint8_t* b, int64_t t0, int64_t Tb, int64_t C, int max_lag,
                      int tolerance, const int32_t* grp, int G, const int32_t* sgrp, int G2, const int32_t* cls, int R,
                      uint32_t* state, uint32_t* cell_cnt, uint32_t* lag_cnt, uint64_t* sec_cnt, uint8_t* mask,
                      uint64_t* status);

/* Lagged composites (superposed-epoch analysis) of a float field around the onsets or the ends of the events of a presence
 * field: what another variable did before, during and after the events of a cell (the driver studies that follow Hobday et
 * al. 2016, 2018; the reference leaves it to host loops over cells).
 *
 * marex_event_composites_u8: x uint8 and v float32, both [Tr][C], are the rows r0 .. r0 + Tr - 1 of a record of T steps; a
 *   cell is present where the byte of x is not 0.  An event of a cell is a maximal run of consecutive present steps.  With
 *   anchor == 0 the anchors of a cell are its onsets, the steps s > 0 with x[s] and not x[s - 1]; with anchor == 1 its ends,
 *   the steps e < T - 1 with x[e] and not x[e + 1].  A run that touches step 0 has no onset and one that touches step T - 1
 *   no end: its true date is unknown, so it is censored.  The call handles the anchors at the steps a .. b - 1; with
 *   L = max_lag (0 .. 30) and H = max(L, 1) the rows must cover max(0, a - H) .. min(T, b + H) - 1.  The rows outside
 *   a .. b - 1 are read but own no anchors: they stand in the place of a carried state, and the accumulators are the only
 *   thing a call continues.  a == b does nothing (and needs no rows).
 *   Per anchor t of cell c under the label g = grp[t] (grp int32 [T], indexed by the global step; NULL with G == 1: every
 *   step is group 0): anchors[g][c] += 1 (uint32 [G][C]), and for every lag l = -L .. L whose step t + l lies in 0 .. T - 1
 *   and whose value a = v[t + l][c] is finite (neither NaN nor +-inf), at j = l + L: cnt[g][c][j] += 1,
 *   sum[g][c][j] += (double)a, sumsq[g][c][j] += (double)a * (double)a.  cnt uint32, sum and sumsq float64, all
 *   [G][C][2 L + 1]: cell-major, the lags of a cell are contiguous.  An anchor under a label outside 0 .. G - 1 addresses
 *   nothing and adds 1 to status[0] (uint64 [1]).  The function only continues anchors, sum, sumsq, cnt and status: the
 *   caller zeroes them before the first window.
 *   Arithmetic: for each (group, cell, lag) the terms are added in ascending anchor step by sequential float64 additions;
 *   the product of two float32 values is exact in float64, so the square carries no rounding of its own.  The counts are
 *   exact integers.  No result depends on the windows or on the layout: a wave owns 64 consecutive cells, finds their
 *   anchors row by row with a ballot, and for every anchor its lanes become the lags (one plain read-modify-write per lane);
 *   only the owning wave touches a cell's accumulators, in time order.  No atomic touches a per-cell output.
 *   -1, with nothing launched: null x, v, anchors, sum, sumsq, cnt or status, C <= 0, G <= 0, NULL grp with G != 1, max_lag
 *   outside 0 .. 30, anchor outside 0 .. 1, not (0 <= r0, 0 <= Tr, r0 + Tr <= T and 0 <= a <= b <= T), rows that do not cover
 *   the halo, a pointer not aligned to its element; -4: C or T of 2^31 - 1 or more (the fields themselves may hold any
 *   number of cells: rows are addressed with 64-bit offsets).  Asynchronous on the context's stream. */
int marex_event_composites_u8(marex_ctx* ctx, const uint8_t* x, const float* v, int64_t r0, int64_t Tr, int64_t a, int64_t b,
                              int64_t T, int64_t C, int max_lag, int anchor, const int32_t* grp, int G, uint32_t* anchors,
                              double* sum, double* sumsq, uint32_t* cnt, uint64_t* status);

/* Per-cell trends of a short series of maps: y float64 [G][C], the G maps of C cells (2 <= G <= 256, C below 2^31 - 1),
 * x float64 [G] their finite, strictly increasing abscissae (the caller checks that).  A sample that is not finite is a
 * missing sample of its cell; n is the number of valid ones and P = n (n - 1) / 2 the number of pairs i < j of them.  The
 * slope of a pair is ((y[j] - y[i]) / (x[j] - x[i])) + 0.0: two subtractions, one IEEE division, and the addition that
 * makes -0.0 and +0.0 one value; nothing is contracted.
 *
 * marex_trend_stats_f64, one launch, per cell c: n[c]; s[c] = sum over the pairs of sign(y[j] - y[i]) (Mann-Kendall S);
 *   ties[c] = sum over the valid samples of (t - 1)(2 t + 5), t the number of valid samples equal to it, itself included
 *   (that is sum over the tie groups of t (t - 1)(2 t + 5); -0.0 equals +0.0); med float64 [2][C]: [0] the median of the
 *   valid y, (0.5 * (lower + upper middle of the sorted samples)) + 0.0, found from the counts of smaller and equal
 *   samples without a sort, [1] the same of the x of the valid samples; sums float64 [5][C]: xbar = (sum x) / n,
 *   ybar = (sum y) / n, Sxx = sum (x - xbar)^2, Sxy = sum (x - xbar)(y - ybar), Syy = sum (y - ybar)^2, each sum over the
 *   valid samples in ascending step order by sequential float64 additions of separately rounded products.  A cell with
 *   n == 0 has NaN medians and means and zero sums; status is not touched.
 * marex_trend_select_f64: ranks int32 [K][C], out float64 [K][C] (K >= 1): out[k][c] is the ranks[k][c]-th smallest
 *   (0-based) of the P slopes of cell c, NaN for a rank outside 0 .. P - 1.  The slopes are never stored: a bisection over
 *   the order-preserving 64-bit keys of the doubles between -inf and +inf recomputes them in each of its at most 64 steps
 *   and counts those not above the pivot, each quotient compared with up to four pivots of the cell.  A selection that
 *   has not closed after 64 steps writes NaN and adds 1 to status[1] (int64 [2], continued: the caller zeroes it; [0] is
 *   not used).
 * A lane owns a cell; a wave keeps its 64 cells' samples in LDS up to G = 128 (statistics) or G = 64 (selection) and
 * re-reads y above (same results).  y needs no more than its natural 8-byte alignment.
 * -1: null pointer, G outside 2 .. 256, C <= 0, K <= 0; -4: C of 2^31 - 1 or more.  Asynchronous on the context's stream. */
int marex_trend_stats_f64(marex_ctx* ctx, const double* y, const double* x, int G, int64_t C, int32_t* n, int32_t* s,
                          int32_t* ties, double* med, double* sums, int64_t* status);
int marex_trend_select_f64(marex_ctx* ctx, const double* y, const double* x, int G, int64_t C, const int32_t* ranks, int K,
                           double* out, int64_t* status);

/* Per-(timestep, region) series of an event mask or a tracked ID field: the area in an extreme state, its cells, the
 * weighted anomaly sums, the largest anomaly and the severity categories of every region at every step (the reference
 * leaves them to notebook code: (extreme_events * cell_area).where(basin).sum over space; Hobday et al. 2018, Fig. 3).
 *
 * marex_regional_series_u8 / marex_regional_series_i32: x uint8 / int32 [Tb][C] are the rows t0 .. t0 + Tb - 1 of a [T][C]
 *   field, T = T_slots >= t0 + Tb.  A cell is present when x > 0 (match == 0) or when x == match (match > 0); a negative
 *   int32 cell is never present and adds one to status[0].  reg int32 [C]: the region of every cell; a value outside
 *   0 .. R - 1 belongs to no region and adds nothing anywhere.  Slot (t, r) of the global step t = t0 + row is t * R + r.
 *   q int64 [C], or NULL: the fixed-point areas (row 0 of the mesh tracker's weight tables: rint(a 2^e), their sum below
 *   2^62); NULL means 1 per cell, and no weights are loaded.  wf float32 [C], or NULL for 1: the weights of the anomaly
 *   sums (needs anom).  anom float32 [Tb][C] with sums and vmax, or all three NULL.  thr float32 [n_doy][C] with doy int32
 *   [T] (the row of thr of every global step, must reach t0 + Tb) and cat_cnt, or all three NULL (they need anom);
 *   cat_area exactly with thr and q.
 *   Per present cell c of region r at step t:
 *     without anom: area[t][r] += q[c] (int64 [T][R]), cnt[t][r][0] += 1 (uint64 [T][R][2]);
 *     with a finite anomaly a: the same two, sums[t][r][0] += (double)wf[c], sums[t][r][1] += (double)wf[c] * (double)a (an
 *     exact product; float64 [T][R][2]), vmax[t][r] = max(vmax[t][r], key(a)) (uint32 [T][R]; the key of
 *     marex_event_intensity_f32, 0: no finite cell), and with thr the class k of marex_local_intensity_* under h =
 *     thr[doy[t]][c]: cat_cnt[t][r][k] += 1 (uint64 [T][R][6]), cat_area[t][r][k] += q[c] (int64 [T][R][6]);
 *     with an anomaly that is NaN or +-inf: cnt[t][r][1] += 1 and nothing else -- area and cnt[0] count the same cells.
 *   Under a row whose doy label lies outside 0 .. n_doy - 1 nothing is addressed: its present cells of a region add to
 *   status[1] and to nothing else.  status uint64 [2].  The functions only add: the caller zeroes area, cnt, sums, vmax,
 *   cat_cnt, cat_area and status before the first window, and walks a record in any sequence of windows into them.
 *   anom is fetched only under present cells of a region, thr, wf and q only under those of them with a finite anomaly.
 *   Arithmetic: every count and every area is an integer, exact and independent of the order of execution, of the windows
 *   and of the layout below.  sums follows the contract of marex_event_intensity_f32: exact terms, summed in registers,
 *   over the wave, through LDS and by atomic adds in no fixed order; bit for bit reproducible whenever the partial sums are
 *   exactly representable, otherwise within 2 n u sum|w a| of the exact sum (n the finite cells of the slot, u = 2^-53).
 *   Layout: a workgroup of 256 lanes takes 4096 consecutive cells (four per lane and pass; uint8 without thr, with C % 4 == 0, x 4-byte
 *   and anom, wf and q 16-byte aligned) or 2048 (one per lane and pass), a wave a quarter of them, and every 32nd
 *   row; same results either way.
 *   -1: null x, reg, area, cnt or status, empty shape, t0 < 0, T_slots < t0 + Tb, match < 0, R <= 0, anom / sums / vmax or
 *   thr / doy / cat_cnt given in part, wf or thr without anom, n_doy <= 0 with thr, cat_area without thr and q or missing
 *   with both; -4: C or t0 + Tb of 2^31 - 1 or more (the field itself may hold any number of cells: it is addressed with
 *   64-bit offsets).  Asynchronous on the context's stream. */
int marex_regional_series_u8(marex_ctx* ctx, const uint8_t* x, int64_t t0, int64_t Tb, int64_t C, int64_t T_slots, int match,
                             const int32_t* reg, int R, const int64_t* q, const float* wf, const float* anom, const float* thr,
                             const int32_t* doy, int n_doy, int64_t* area, uint64_t* cnt, double* sums, uint32_t* vmax,
                             uint64_t* cat_cnt, int64_t* cat_area, uint64_t* status);
int marex_regional_series_i32(marex_ctx* ctx, const int32_t* x, int64_t t0, int64_t Tb, int64_t C, int64_t T_slots, int match,
                              const int32_t* reg, int R, const int64_t* q, const float* wf, const float* anom, const float* thr,
                              const int32_t* doy, int n_doy, int64_t* area, uint64_t* cnt, double* sums, uint32_t* vmax,
                              uint64_t* cat_cnt, int64_t* cat_area, uint64_t* status);
/* marex_regional_layout: what the kernels of marex_regional_series_* are compiled with, for cells_per_lane 4 or 1: out
 *   int32 [3] (host) = cells of a wave per row, cells of a workgroup per row, rows between two of a workgroup's.  -1: null
 *   out or another cells_per_lane.  Needs no context and no device. */
int marex_regional_layout(int cells_per_lane, int32_t* out);

/* The join of tracked events with regions: per (timestep, region, event) the cells of the event in the region, their area,
 * the weighted anomaly sums and the largest anomaly.  The result is sparse, so it is a keyed accumulation in an
 * open-addressing table (the scheme of marex_overlap_count_i32 / marex_overlap_pairs_i32), not a dense slot array.
 *
 * Both functions take ids int32 [Tb][C], one window of a tracked field (a cell belongs to event ids > 0; a negative cell
 * belongs to none), and reg int32 [C], the region rank of every cell: a value outside 0 .. R - 1 is "no region", which is
 * accumulated under rank R.  The key of a cell is id << 33 | rank << 17 | row (31, 16 and 17 bits): as integers the keys
 * sort by (id, rank, row).  Equal keys of consecutive cells of a row form a run.
 *
 * marex_event_exposure_count_i32: status uint64 [8] is zeroed, then status[0] = negative cells, status[2] = runs (an upper
 *   bound of the distinct keys), status[4] = event cells.
 * marex_event_exposure_i32: every run is added to the entry of its key in a table of cap entries (a power of two >= 64; the
 *   caller chooses cap >= 2 runs), which the function zeroes: keys uint64 [cap] (0 = empty), cnt uint64 [cap] (the cells in
 *   the low and the cells with a finite anomaly in the high 32 bits; without anom every cell is finite), area int64 [cap]
 *   with q int64 [C] (the sum of the fixed-point areas q of the cells, all of them; NULL together: the area is the cells),
 *   and with anom float32 [Tb][C]: sums double [cap][2] (the sum of w and of w * anom over the cells with a finite anomaly,
 *   w = wf float32 [C] or 1 with wf NULL; exact products of doubles, added in no fixed order) and vmax uint32 [cap] (the
 *   largest finite anomaly as an order-preserving key, 0: none).  anom, sums, vmax, out_sums and out_vmax come together or
 *   not at all, q, area and out_area likewise.  A run that finds no entry within cap probes sets status[1] and is dropped:
 *   nothing spins, nothing is written outside the table.  Then the occupied entries are copied, in no particular order, to
 *   out_keys, out_cnt, out_area, out_sums [.][2] and out_vmax (out_cap entries each); status[3] = the occupied entries, of
 *   which only the first out_cap are written.  status[0], [2] and [4] are left as the count pass set them.
 * marex_event_exposure_layout: out int32 [7] (host) = the cells of a piece, of a wave and of a workgroup per row, the rows
 *   between two of a workgroup's, and the bits of the id, the rank and the row in the key.  Needs no context and no device.
 *
 * -1: null pointer, empty shape, R outside 1 .. 32767, cap no power of two >= 64, out_cap <= 0, arguments given in part;
 * -4: Tb above 2^17 or C of 2^31 - 1 or more.  Asynchronous on the context's stream. */
int marex_event_exposure_count_i32(marex_ctx* ctx, const int32_t* ids, int64_t Tb, int64_t C, const int32_t* reg, int R,
                                   uint64_t* status);
int marex_event_exposure_i32(marex_ctx* ctx, const int32_t* ids, int64_t Tb, int64_t C, const int32_t* reg, int R,
                             const int64_t* q, const float* wf, const float* anom, int64_t cap, uint64_t* keys, uint64_t* cnt,
                             int64_t* area, double* sums, uint32_t* vmax, uint64_t* status, int64_t out_cap, uint64_t* out_keys,
                             uint64_t* out_cnt, int64_t* out_area, double* out_sums, uint32_t* out_vmax);
int marex_event_exposure_layout(int32_t* out);

/* The join of two tracked fields: per (timestep, event of A, event of B) the cells that the two share and their area, by the
 * scheme of the exposure functions above with a second streamed field in the place of the region map.
 *
 * Both functions take ids_a and ids_b int32 [Tb][C], one window of two tracked fields over the same cells (a cell belongs to
 * event ids > 0 of its field; a negative cell belongs to none).  A cell is present where either field holds an event; the
 * pairs (a, 0) and (0, b), the cells of an event that the other field leaves uncovered, are kept like any other, and no pair
 * is (0, 0).  The key of a cell is a << (bits_b + bits_step) | b << bits_step | row with widths that the caller passes at
 * run time: one 64-bit word for one compare-and-swap, never two words, a lock or a spin.  As integers the keys sort by
 * (a, b, row).  Equal pairs of consecutive cells of a row form a run.
 *
 * marex_event_matching_count_i32: status uint64 [8] is zeroed, then status[0] = negative cells of A, status[1] = negative
 *   cells of B, status[2] = runs (an upper bound of the distinct keys), status[3] = the largest ID of A, status[4] = the
 *   largest ID of B (0: none): what the caller plans the widths and the table from.
 * marex_event_matching_i32: every run is added to the entry of its key in a table of cap entries (a power of two >= 64; the
 *   caller chooses cap >= 2 runs), which the function zeroes: keys uint64 [cap] (0 = empty), cnt uint64 [cap] (the cells),
 *   and area int64 [cap] with q int64 [C] (the sum of the fixed-point areas q of the cells, read under present cells only;
 *   q, area and out_area come together or not at all).  The widths must each be at least 1 and sum to at most 64, and Tb
 *   at most 2^bits_step.  A run whose a needs more than bits_a bits, or whose b more than bits_b, adds its cells to
 *   status[6] and is dropped before a key is formed: it is never mis-keyed.  A run that finds no entry within cap probes
 *   sets status[5] and is dropped: nothing spins, nothing is written outside the table.  Then the occupied entries are
 *   copied, in no particular order, to out_keys, out_cnt and out_area (out_cap entries each); status[7] = the occupied
 *   entries, of which only the first out_cap are written.  status[0] .. [4] are left as the count pass set them.
 * marex_event_matching_layout: out int32 [6] (host) = the cells of a piece, of a wave and of a workgroup per row, the rows
 *   between two of a workgroup's, the most bits an ID takes (31) and the fewest that remain for the row (2).  Needs no
 *   context and no device.
 *
 * -1: null pointer, empty shape, widths below 1 or above 64 together, cap no power of two >= 64, out_cap <= 0, area
 * arguments given in part; -4: Tb above 2^bits_step or C of 2^31 - 1 or more.  Asynchronous on the context's stream. */
int marex_event_matching_count_i32(marex_ctx* ctx, const int32_t* ids_a, const int32_t* ids_b, int64_t Tb, int64_t C,
                                   uint64_t* status);
int marex_event_matching_i32(marex_ctx* ctx, const int32_t* ids_a, const int32_t* ids_b, int64_t Tb, int64_t C,
                             const int64_t* q, int bits_a, int bits_b, int bits_step, int64_t cap, uint64_t* keys,
                             uint64_t* cnt, int64_t* area, uint64_t* status, int64_t out_cap, uint64_t* out_keys,
                             uint64_t* out_cnt, int64_t* out_area);
int marex_event_matching_layout(int32_t* out);

/* The partition kernels of the split-and-merge stage on an unstructured mesh (tracker.split_and_merge_objects_parallel,
 * marEx/track.py:3804-4814, 5246-5419).  A slice is int32 [C], values <= 0 are background, C below 2^31 - 1.  u: float64
 * [3][C], the unit vectors of the cells; pv: float64 [3][n], the unit vectors of the parents' centroids.  "Nearest" is the
 * smallest ((dx dx + dy dy) + dz dz) in float64 without fused multiply-add, first minimum.
 *
 * marex_mesh_partition_centroid_i32: every cell of child child_keys[k] (ascending, distinct) takes lab[j] of the nearest
 *   of the parent entries j in off[k] .. off[k + 1] (of n_ent).  In place, all merging children of one timestep at once.
 * marex_mesh_nn_seed_i32 / marex_mesh_nn_hops_i32 / marex_mesh_nn_finish_i32 (partition_nn_unstructured_optimised) for one
 *   child of the slice cur, with parents[j] (n_par <= 10) the parent IDs in the slice prev.  word: uint32 [C] work, one
 *   (substep stamp << 8 | owner) per cell, owner 255 = unclaimed.  ctl: int32 [8]: [0] child cells without an owner,
 *   [1] a child cell was claimed in the running hop, [2] stopped, [3] hops run, [4] child cells resolved by the nearest
 *   centroid, [5] why it stopped (1: no child cell left, 2: a hop claimed no child cell, 3: max_hops).  seed zeroes ctl,
 *   gives the cells of parent j the owner j and counts ctl[0].  hops queues hops first_hop .. first_hop + n_hops (at most
 *   max_hops in all; nbr: int32 [3][C], 0-based, negative = none): before each hop one thread applies the stopping
 *   rule; a hop is one launch per (parent ascending, direction 0 .. 2), in which every unclaimed cell that is the
 *   listed neighbour of a cell the parent owned when the launch began becomes the parent's; launches after ctl[2] was
 *   set do nothing, so the caller may read ctl as rarely as it likes.  finish applies the stopping rule once more and
 *   writes cur[c] = lab[owner] on the child's cells, unclaimed ones by the nearest of pv [3][n_par].
 * All are asynchronous on the context's stream. */
int marex_mesh_partition_centroid_i32(marex_ctx* ctx, int32_t* ids, int64_t C, const int32_t* child_keys, int n_child,
                                      const int32_t* off, const double* u, const double* pv, int n_ent, const int32_t* lab);
int marex_mesh_nn_seed_i32(marex_ctx* ctx, const int32_t* cur, const int32_t* prev, int64_t C, int child,
                           const int32_t* parents, int n_par, uint32_t* word, int32_t* ctl);
int marex_mesh_nn_hops_i32(marex_ctx* ctx, const int32_t* cur, const int32_t* nbr, int64_t C, int child, int n_par,
                           int first_hop, int n_hops, int max_hops, uint32_t* word, int32_t* ctl);
int marex_mesh_nn_finish_i32(marex_ctx* ctx, int32_t* cur, int64_t C, int child, const double* u, const double* pv, int n_par,
                             const int32_t* lab, const uint32_t* word, int32_t* ctl, int max_hops);

/* out[c, r] = in[r, c]  (thresholds [366, C] -> the reference's (cells, dayofyear) order) */
int marex_transpose_f32(marex_ctx* ctx, const float* in, int64_t rows, int64_t cols, float* out);

#ifdef __cplusplus
}
#endif
#endif /* MAREX_HIP_H */
