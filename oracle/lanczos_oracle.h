/*
 * oracle/lanczos_oracle.h -- CPU restatement of the reference's *software* Lanczos path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under lanczos-hls_amd/ (the product) may include,
 * link or call this.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
 * leg use it, and only as the checker / the timed CPU baseline.
 *
 * What it restates (all in /root/reference/LanczosUpscaler/full_TB.h):
 *   double_to_uint8          :29-37   clamp to [0,255] then C-cast (truncate)
 *   sinc                     :39-44   x==0 ? 1 : sin(x)/x
 *   lanczos_kernel(double)   :51-53   sinc(pi*x) * sinc(pi*x/a), no |x|<a window test
 *   lanczos_interpolate_row  :55-65   H pass, truncating u8 store
 *   lanczos_interpolate_col  :67-77   V pass, IN PLACE, descending output row
 *   lanczos_expected         :79-96   H pass over rows 0..IN_H-1, then V pass per column
 * with SCALE = (double)SCALE_N/SCALE_D (lanczos.h:112) and MIN/MAX (lanczos.h:63-64).
 *
 * Parity pin: checked bit-for-bit against (a) the five FNV-1a-64 digests recorded in
 * SURVEY.md 8(c) and (b) the reference's own lines compiled by oracle/build_ref.sh
 * (tests/test_oracle.py, tests/golden/).  Build with -ffp-contract=off.
 */
#ifndef LANCZOS_ORACLE_H
#define LANCZOS_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int in_w, in_h;     /* IN_WIDTH, IN_HEIGHT   */
    int out_w, out_h;   /* OUT_WIDTH, OUT_HEIGHT */
    int channels;       /* NUM_CHANNELS          */
    int a;              /* LANCZOS_A             */
    int scale_n, scale_d; /* SCALE_N, SCALE_D    */
} oracle_cfg;

/* full_TB.h:51-53 with LANCZOS_A as an argument */
double oracle_lanczos_kernel(double x, int a);
/* full_TB.h:29-37 */
uint8_t oracle_double_to_uint8(double x);

/* full_TB.h:79-96 on the reference's planar layout: in[C][IN_H][IN_W] -> out[C][OUT_H][OUT_W].
 * threads <= 1: the reference's single-threaded loop order.  threads > 1: H-pass rows and V-pass
 * columns are split across pthreads (rows/columns are independent, so results are identical). */
int oracle_expected_planar_u8(const oracle_cfg* cfg, const uint8_t* in, uint8_t* out, int threads);

/* Same computation on the stb interleaved HWC layout the harness hands over (full_TB.h:127-138
 * planar<->interleaved glue folded in). */
int oracle_expected_hwc_u8(const oracle_cfg* cfg, const uint8_t* in, uint8_t* out, int threads);

/* 16-bit generalisation (clamp 65535, truncation).  NOT expressible in the reference (byte is 8 bit,
 * full_TB.h:18,30): "parity unpinned" -- it is this same code path templated on the sample type. */
int oracle_expected_hwc_u16(const oracle_cfg* cfg, const uint16_t* in, uint16_t* out, int threads);

/* Out-of-place V pass (what a naive resampler would do) -- used by tests to show where the
 * in-place quirk (rows < K) matters.  Not a reference behaviour. */
int oracle_outofplace_hwc_u8(const oracle_cfg* cfg, const uint8_t* in, uint8_t* out);

/* First output row not affected by the in-place V pass: K = min{y : y - floor(y/S) >= a}. */
int oracle_inplace_rows(const oracle_cfg* cfg);

/* The truncated horizontal intermediate T[IN_H][OUT_W][C] exactly as the reference holds it before the V pass
 * (full_TB.h:83-87: rows 0..IN_H-1 of the output plane).  Test infrastructure for the LSB1 check below. */
int oracle_hpass_hwc_u8(const oracle_cfg* cfg, const uint8_t* in, uint8_t* T, int threads);
int oracle_hpass_hwc_u16(const oracle_cfg* cfg, const uint16_t* in, uint16_t* T, int threads);

/* What oracle_explain_hwc_* found.  v is the reference's f64 vertical sum of a sample (full_TB.h:67-77), store() its
 * clamp-and-truncate store; "reference" below is store(v). */
typedef struct {
    uint64_t samples;
    uint64_t equal;            /* got == store(v) */
    uint64_t plus1;            /* got == store(v) + 1 and explained: v lies within delta below got */
    uint64_t unexplained;      /* see first_kind */
    uint64_t window;           /* rows >= K that are not integer-phase rows: store(v - delta) != store(v + delta) -- where a
                                  delta error could change the store (an integer-phase row's v is T[i] itself, +- 1e-17) */
    uint64_t int_flips;        /* integer-phase H samples (x = xx / SCALE an exact integer) whose truncated store differs
                                  from the input sample under them (the double-noise flips of SURVEY.md Q4) */
    uint64_t int_row_samples;  /* samples of integer-phase output rows >= K checked against T's row byte for byte */
    double max_plus1_gap;      /* largest got - v over the explained +1 samples (the error the f32 chain actually used) */
    int inplace_rows;          /* K */
    int first_o, first_x, first_c;  /* the first unexplained sample in memory order, -1 if none */
    int first_kind;            /* 1: outside [store(v), store(v + delta)]; 2: a row < K that is not store(v);
                                  3: an integer-phase row >= K that is not a copy of T's row */
    long long first_got;
    double first_v;
} oracle_explain_stats;

/* Classify a candidate HWC output `got` of a reference-model request.  A sample of a row o >= K is explained iff
 * store(v) <= got <= store(v + delta) (the kernels store floor(sum + eps) with |sum - v| <= eps, so they never land below
 * store(v)); rows o < K must equal store(v) (the prefix kernels are f64 throughout); copies_int_rows != 0 adds: an
 * integer-phase row o >= K (x = o / SCALE the exact integer i) equals T's row i.  ref_out (may be NULL) receives store(v),
 * which is the reference's output.  Returns 0, or < 0 on a bad argument / no memory. */
int oracle_explain_hwc_u8(const oracle_cfg* cfg, const uint8_t* in, const uint8_t* got, double delta, int copies_int_rows,
                          oracle_explain_stats* stats, uint8_t* ref_out, int threads);
int oracle_explain_hwc_u16(const oracle_cfg* cfg, const uint16_t* in, const uint16_t* got, double delta,
                           int copies_int_rows, oracle_explain_stats* stats, uint16_t* ref_out, int threads);

/* Helpers shared by tests: FNV-1a-64 and the LCG byte generator of SURVEY.md 8(c). */
uint64_t oracle_fnv1a64(const void* data, size_t n);
void oracle_lcg_fill_u8(uint8_t* dst, size_t n, uint32_t seed);
void oracle_lcg_fill_u16(uint16_t* dst, size_t n, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif
