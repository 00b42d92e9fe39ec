/*
 * fractal_hip.h — C ABI of libfractal_hip.so, the MI355X (gfx950) implementation of
 * Icelk/fractal-renderer's escape-time hot path.
 *
 * The reference is pure Rust and has NO FFI of its own; the seam this library fills is the
 * three public functions + four types of the `calc` crate and the host library's get_image:
 *
 *   pub fn recursive(iterations, start, c, limit) -> (Imaginary, u32)   calc/src/lib.rs:245
 *   pub fn get_recursive_pixel(&Config, x, y) -> RGB                    calc/src/lib.rs:199
 *   pub fn get_image(&Config) -> Vec<RGB>   (Mandelbrot | Julia arm)    src/lib.rs:253-270
 *   Config / Imaginary / RGB / Algo                                     calc/src/lib.rs:21-37,79-82,121-125,150-154
 *
 * Every entry point below names the reference interface it replaces.  INTEGRATION.md shows the
 * Rust `extern "C"` block and the patch to src/lib.rs:253-270 a maintainer would add.
 *
 * Conventions
 *   - Plain pointers and sizes only.  The CALLER owns every buffer; the library never frees or
 *     keeps a caller pointer past the call.
 *   - Every function returns FR_OK (0) or an fr_status error code and never aborts the process;
 *     fr_last_error() returns a thread-local message for the last failing call on this thread.
 *     (The reference's get_image is infallible; the Rust shim maps an error to a panic or to its
 *     own CPU arm — INTEGRATION.md.)
 *   - Re-entrant: may be called concurrently from several host threads with different configs,
 *     as the GUI's render thread and screenshot thread do (src/gui.rs:56-60, 322-326).
 *   - Output pixel layout is the reference's Vec<RGB>: row-major, tightly packed bytes r,g,b;
 *     pixel (x, y) of the image lives at byte 3*(y*width + x).
 *   - There is no CPU fallback: without a usable gfx950 device every compute call fails with
 *     FR_ERR_NO_DEVICE.
 *
 * STREAM ORDER — the contract of every entry point with a `void *hip_stream` parameter (a hipStream_t; NULL = the null stream),
 * stated once; the per-call comments say "asynchronous on `hip_stream`" and mean this.
 *   - ALL device work of the call — every kernel, every memset (the adaptive calls' counters, the survivor lists' and the
 *     statistics' zeroing) and every device-to-device copy — is enqueued on `hip_stream`, in the order the call's definition
 *     needs, and on no other stream (but for a cache miss's own copies, below): work the caller queued on that stream before the call (filling the inputs, an earlier call
 *     that writes the state) is finished before the call's work starts, and work queued behind it sees its results.  This holds on
 *     a non-blocking stream (hipStreamNonBlocking), which does not synchronise with the null stream.  The call returns without
 *     waiting for the stream and allocates no device memory, with these exceptions, all bounded by work already queued:
 *       a CACHE MISS — a PT, BLA-PT or SCALED PT call whose view's orbit or table the context does not hold (a new view, or a
 *         higher cap that CONTINUES the cached orbits) computes it on the host, uploads it synchronously and frees the one it
 *         replaces, which waits for the device.  This is the one place where device work is NOT on `hip_stream`: a continuation
 *         copies the entries it keeps device-to-device on the NULL stream and the host waits for that stream before anything is
 *         launched, so the copies are complete — like the synchronous upload — before the call enqueues its first kernel;
 *       a FULL RING — a render that finds the 16 palette / counter slots or the 3 survivor-list buffers all in flight waits for
 *         the oldest one's event;
 *       the FIRST TWO-PASS GROWTH — the first two-pass render that needs survivor lists larger than any before reallocates them;
 *       and, on F64 / F32, the first render of a view of 131 072 tiles and more, which takes one blocking 40 us sample.
 *   - Until the stream has drained the caller keeps alive, and does not touch from another stream, every DEVICE buffer it
 *     passed: outputs, the kept arrays a call reads or continues in place, and the workspace it lends (which holds the call's
 *     lists and their counters).  Host arguments (cfg, pos_lo, the centre's words, opts) are read before the call returns.
 *   - fr_render_rgb8_multi_device takes no stream: it renders on streams of its own (see there).
 *   tests/test_gpu_stream_order.py holds every such entry point to this behind a gate on a non-blocking stream.
 */
#ifndef FRACTAL_HIP_H
#define FRACTAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_ABI_VERSION 3

typedef enum fr_status {
    FR_OK = 0,
    FR_ERR_INVALID_ARGUMENT = 1, /* NULL pointer, y0 > y1, y1 > height, ... */
    FR_ERR_BUFFER_TOO_SMALL = 2, /* out_len < bytes the call must write */
    FR_ERR_NO_DEVICE = 3,        /* no HIP device / not initialised and auto-init failed */
    FR_ERR_HIP = 4,              /* a HIP runtime call failed; see fr_last_error() */
    FR_ERR_UNSUPPORTED_ALGO = 5  /* reserved; Algo::BarnsleyFern is NOT an error (renders black) */
} fr_status;

/* enum Algo — calc/src/lib.rs:150-154, in declaration order */
typedef enum fr_algo {
    FR_ALGO_MANDELBROT = 0,
    FR_ALGO_BARNSLEY_FERN = 1, /* on this path: every pixel RGB::BLACK (calc/src/lib.rs:211) */
    FR_ALGO_JULIA = 2
} fr_algo;

/* struct Imaginary — calc/src/lib.rs:79-82 */
typedef struct fr_imaginary {
    double re;
    double im;
} fr_imaginary;

/* struct RGB — calc/src/lib.rs:121-125.  These are the STORED fields.  RGB::new(r, b, g) takes
 * blue second (calc/src/lib.rs:129-131), so e.g. Config::new's RGB::new(40, 40, 255) is stored
 * {r:40, g:255, b:40}; pass the stored struct verbatim — the library reproduces color_multiply's
 * swap (calc/src/lib.rs:133-139) internally. */
typedef struct fr_rgb {
    uint8_t r;
    uint8_t g;
    uint8_t b;
} fr_rgb;

/* struct Config — calc/src/lib.rs:21-37, field for field (`#[repr(C)]` image; bools as u8,
 * enum as u32).  sizeof == 104. */
typedef struct fr_config {
    uint32_t algo; /* fr_algo */
    uint32_t width;
    uint32_t height;
    uint32_t iterations;
    double limit;        /* escape RADIUS; squared inside recursive() (calc/src/lib.rs:246) */
    double stable_limit; /* compared with the SQUARED distance, un-squared (calc/src/lib.rs:216) */
    fr_imaginary pos;
    fr_imaginary scale; /* per-axis pair, not a complex number */
    double exposure;
    uint8_t inside;
    uint8_t smooth;
    fr_rgb primary_color;
    fr_rgb secondary_color;
    double color_weight; /* fern only; ignored on this path */
    fr_imaginary julia_set;
} fr_config;

/* Arithmetic of the z = z^2 + c loop.  F64 is the reference's (and the only one with a parity
 * claim against it).  F32 is this build's fast path for shallow zooms, defined as: coordinates
 * (calc/src/lib.rs:181-197) in f64, start / c / limit narrowed to f32, recursive() evaluated in
 * f32 with the same operation order, final position widened to f64, colour mapping in f64. */
/*
 * DD (double-double) is for zooms past the f64 limit: once a pixel is narrower than about one f64 ulp of pos (scale
 * >~ 10^13 near |pos| ~ 0.75 at 1080 rows) neighbouring pixels get the same f64 start and the image turns into flat
 * blocks.  A dd is a pair (hi, lo) of f64 values (about 106-bit significands).  DD is DEFINED by this exact operation
 * sequence (each fma one correctly rounded fused multiply-add, nothing else fused):
 *   two_sum(a,b):      s = a+b; bb = s-a; e = (a-(s-bb)) + (b-bb)                              -> (s, e)
 *   fast_two_sum(a,b): s = a+b; e = b-(s-a)                                                    -> (s, e)
 *   add_dd(a,b):       (sh,sl) = two_sum(a.hi,b.hi); (th,tl) = two_sum(a.lo,b.lo)
 *                      sl = sl+th; (sh,sl) = fast_two_sum(sh,sl); sl = sl+tl; (sh,sl) = fast_two_sum(sh,sl)
 *   add_d(a,d):        (sh,sl) = two_sum(a.hi,d); sl = sl+a.lo; (sh,sl) = fast_two_sum(sh,sl)
 *   sqr(x):            p = x.hi*x.hi; e = fma(x.hi,x.hi,-p); e = fma(x.hi+x.hi, x.lo, e); fast_two_sum(p,e)
 *   twice_mul(x,y):    p = x.hi*y.hi; e = fma(x.hi,y.hi,-p); e = fma(x.hi,y.lo,e); e = fma(x.lo,y.hi,e)
 *                      (h,l) = fast_two_sum(p,e); -> (h+h, l+l)
 *   negation negates both halves.
 * Start: off_re = ((x/h) - ((w/h)/2)) / scale.re, off_im = ((y/h) - 0.5) / scale.im (one f64 operation each, in this
 * order: coord_to_space without the final + pos), start = add_d((pos, pos_lo), off) per axis.  With pos_lo = 0,
 * start.hi is the f64 start bit for bit.
 * One iteration: re' = add_dd(add_dd(sqr(re), -sqr(im)), c.re), im' = add_dd(twice_mul(re, im), c.im); Mandelbrot:
 * c = start (dd); Julia: c = julia_set (f64) and the two outer add_dd are add_d.
 * Escape test and loop semantics are recursive()'s (calc/src/lib.rs:245-257) with dist = re'.hi*re'.hi + im'.hi*im'.hi
 * and dist > limit*limit in f64: on escape `next` with index i, on exhaustion `previous` with `iterations`.
 * Colour: the colour map applied to the hi parts (r2 = re.hi*re.hi, i2 = im.hi*im.hi): fr_colour_rgb8 over the hi
 * parts of fr_escape_rows(_dd) reproduces the DD image.
 * Domain (else FR_ERR_INVALID_ARGUMENT, before any device work): every double field of the config and of pos_lo finite;
 * 0 < limit <= 2^500; |pos|, |julia_set| <= 2^64 and |scale| >= 2^-64 on either axis; pos_lo normalised
 * (pos.re + pos_lo.re == pos.re in f64, same for im).  This keeps every hi product finite up to the escape test.
 * DD runs on one device: the single-device row renders, fr_pixel_p, fr_escape_rows (hi parts), fr_count_iterations
 * (all with pos_lo = 0) and the fr_*_dd calls below take it; block-cyclic, multi-device and fr_recursive_batch do not.
 * Implementation selectors (fr_set_tile, fr_render_opts, ...) select nothing for DD: it has one kernel. */
/*
 * PT (perturbation) is DD's deep zoom at near-f64 cost for long orbits: one reference orbit per view in dd, stored as its
 * f64 hi parts, and each pixel iterates in f64 only its offset from that orbit (with rebasing, so one orbit serves every
 * pixel).  PT is DEFINED by this exact operation sequence (the dd operations are DD's above):
 *   C = (pos, pos_lo) as a dd; off = DD's off (one f64 operation each, as above); a pixel's point is C + off.
 *   Reference orbits, each iterated in dd with DD's operations of one iteration, stored as (re.hi, im.hi) per entry:
 *     Mandelbrot R: R_0 = 0, R_1 = C, R_{k+1} = add_dd(add_dd(sqr(R_k.re), -sqr(R_k.im)), C.re),
 *                                              add_dd(twice_mul(R_k.re, R_k.im), C.im)
 *     Julia V (view orbit): V_0 = C, V_{k+1} = add_d(add_dd(sqr(V_k.re), -sqr(V_k.im)), J.re), add_d(twice_mul(..), J.im)
 *     Julia K (critical orbit): K_0 = 0, K_{k+1} = the same with K for V          (J = julia_set, f64)
 *   An orbit X stores entries X_0 .. X_last: it stops at the first k >= kmin whose stored hi parts have
 *   re*re + im*im > 4 (f64), else at k = kmax.  R: kmin = 2, kmax = iterations + 1; V and K: kmin = 1,
 *   kmax = max(iterations, 1).
 *   Pixel state (X, m, z, dz, dc): the orbit followed, an index into it, the f64 position z and its offset dz from X_m.
 *     Mandelbrot: X = R, m = 1, dz = off, dc = off.  Julia: X = V, m = 0, dz = off, dc = 0.  Then z = X_m + dz (f64).
 *   Step i = 0 .. iterations-1:
 *     t   = X_m + z                                                       (per axis: 2 X_m + dz of z' = z^2 + c)
 *     dz' = (fma(t.re, dz.re, fma(-t.im, dz.im, dc.re)), fma(t.re, dz.im, fma(t.im, dz.re, dc.im)))
 *     m   = m + 1;  z' = X_m + dz' (per axis, f64);  z = z', dz = dz'
 *     dist = z.re*z.re + z.im*z.im: dist > limit*limit -> escape with (z, i), as recursive() (calc/src/lib.rs:245-257)
 *     else rebase when dist < dz.re*dz.re + dz.im*dz.im or m == last of X: dz = z, m = 0 (z unchanged); Julia then
 *     follows K (and stays on K).
 *   Exhaustion: (z, iterations).  Colour: the colour map on the f64 z (r2 = z.re*z.re, i2 = z.im*z.im):
 *   fr_colour_rgb8 over fr_escape_rows(_pt) reproduces the PT image.
 * Domain: DD's (with its messages naming FR_PRECISION_PT), plus iterations <= FR_PT_MAX_ITERATIONS: the orbit takes
 * 16 B per entry in host and device memory, so the cap bounds one orbit to 256 MiB (512 MiB for a Julia view's two).
 * PT runs on one device exactly where DD does (pos_lo = 0 through fr_render_rows_rgb8 & co), plus the fr_*_pt calls
 * below; block-cyclic, multi-device and fr_recursive_batch refuse it.  The library keeps the last view's orbit per
 * context, so frames of one view, row pieces and fr_pixel_p do not recompute it.
 *
 * RESUMABLE PT (fr_escape_rows_pt_state, fr_escape_extend_pt below): the state that lets a PT view's cap be raised in place.
 *   An orbit X (R, V or K) is ENDED BY ESCAPE if its last stored entry stopped it by the escape test (last >= kmin and
 *   re*re + im*im > 4 on the stored hi parts); otherwise it is CUT BY THE CAP, at k == kmax.  An orbit ended by escape is
 *   identical at every cap >= its length; an orbit cut at cap N is a proper prefix of the orbit at any cap M > N.
 *   The resumable state of a pixel after N steps is (z, dz, m, onK), produced by the step sequence above with ONE change,
 *   to the rebase condition: rebase when dist < |dz|^2, or when m == last of X AND X is ended by escape.
 *   Stored form: z (2 doubles, as fr_escape_rows_pt gives it), iters, dz (2 doubles), m as uint32 whose bit 31 is set when
 *   a Julia pixel follows K (never for Mandelbrot).  An escaped pixel stores dz = (0, 0), m = 0.  N = 0 stores the initial
 *   state (Mandelbrot: m = 1, dz = off; Julia: m = 0, dz = off; z = X_m + dz).
 *   CLAIM: for every N, z and iters of the state run equal PT's at cap N bit for bit, and continuing the state from N for
 *   M - N steps on the orbits of cap M gives the state run at cap M, bit for bit in all four arrays.
 *   Why: after step i, m <= i + 2 (Mandelbrot) or i + 1 (Julia on V), and on K after a rebase m <= N - 1; an orbit cut by
 *   the cap has last = N + 1 (R) or N (V, K).  So on a cut orbit m == last can only be met at the final step i = N - 1, by
 *   a pixel that never rebased.  There PT's rebase changes (dz, m) and leaves z alone: it is invisible in PT's output, and
 *   it is the only event of the sequence that depends on the cap.  The state rule leaves it out, so a state run to N is
 *   a prefix of the state run to M; an orbit ended by escape and the dist test do not depend on the cap at all.
 *
 * WIDE PT (the fr_*_pt_wide calls below): PT past a scale of 10^30.  A dd centre says ~106 bits about where the view is;
 * nothing else in PT has that limit (off is one f64 division; the pixel loop sees only off and the stored f64 entries).  WIDE
 * PT is PT's definition with ONE replacement, the reference orbits, which are iterated in fixed point from a wide centre:
 *   A wide number is n little-endian uint64_t words in two's complement, 2 <= n <= FR_WIDE_MAX_WORDS; its value is
 *   I / 2^F with F = 64 n - 8 (8 integer bits including the sign, so the range is [-128, 128)).
 *   mul(a, b) = floor(a b / 2^F) and mul2(a, b) = floor(2 a b / 2^F), on the exact integer product (an arithmetic shift);
 *   additions and subtractions are exact.
 *   C = (Cre, Cim) is the centre (fr_wide_centre); J = (floor(julia_set.re 2^F), floor(julia_set.im 2^F)).
 *   One step: next(X, A) = (mul(X.re, X.re) - mul(X.im, X.im) + A.re, mul2(X.re, X.im) + A.im).
 *   Orbits: R: R_0 = 0, R_1 = C, R_{k+1} = next(R_k, C).  V: V_0 = C, V_{k+1} = next(V_k, J).  K: K_0 = 0,
 *   K_{k+1} = next(K_k, J).
 *   A stored entry is the f64 nearest to I / 2^F (ties to even), per axis.
 *   Applied to the stored f64 entries, word for word PT's: the stop rule with kmin and kmax, "ended by escape" and "cut by
 *   the cap", the pixel state and the step sequence, the state rule of RESUMABLE PT (with its claim), the colour.
 *   cfg->pos is not read.
 *   Fixed point cannot overflow: an entry that does not stop its orbit has re*re + im*im <= 4 on its stored values, so each
 *   component is at most 2 + 2^-51 in magnitude and the next entry is below 5 + 5 + 3 < 16; an entry that is not tested
 *   (k < kmin: R_1 = C, V_0 = C, and 0) has components within [-2, 2], and what follows it is below 8 + 3 < 16 as well.
 *   The range is 128.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): PT's domain on the remaining fields
 * (finite, 0 < limit <= 2^500, |scale| >= 2^-64, iterations <= FR_PT_MAX_ITERATIONS); every component of the centre and of
 * julia_set within [-2, 2]; n in 2 .. FR_WIDE_MAX_WORDS with non-NULL words; |scale| <= 2^440 on both axes — past about 2^458
 * the squares of the rebase test, |dz|^2 of an off that is 2^-53 of the pixel spacing, leave f64's normal range, and a scaled
 * pixel loop is not part of this definition; and F >= e + 64, where max(|scale.re|, |scale.im|) = f 2^e with 0.5 <= f < 1:
 * the orbit carries 64 guard bits beyond the pixel spacing.  A centre too coarse for its scale is the caller's mistake and
 * is refused, not rendered as a flat image.  One device; block-cyclic and multi-device renders do not take a wide centre, nor does
 * fr_render_rows_ss: supersampling with a wide centre is fr_render_rows_ss_pt(_device).
 *
 * BLA-PT (the fr_*_pt_bla calls below): PT with bilinear-approximation skips.  While a pixel's offset dz from the reference
 * orbit is far smaller than the orbit itself, the step dz' = (2 X_m + dz) dz + dc is linear in (dz, dc) to below f64 rounding,
 * and 2^k composed linear steps are one tabulated dz' = A dz + B dc.  BLA-PT is an APPROXIMATION of PT (how close: DESIGN.md,
 * "BLA-PT") and, like every mode here, is DEFINED exactly: PT's definition (WIDE PT's when a wide centre is given) with one
 * change to the pixel loop, some steps being replaced by table skips.  The reference orbits and their stop rule, off, dc, the
 * pixel's initial state, the plain step, the escape test, the rebase rule (dist < |dz|^2 or m == last) and the colour map on
 * the f64 z are PT's, word for word.  Every operation below is one correctly rounded f64 operation; fma is fused and nothing
 * else is; sqrt is IEEE.
 *   Constants of a view: eps = 2^-bits with bits in 24 .. 53 (FR_BLA_DEFAULT_BITS = 40); b0 = 1 for Mandelbrot, 0 for Julia
 *   (dc = 0 there); D bounds |dc| over the WHOLE image, not the rows of a call, so row pieces agree:
 *     mr = max(|off_re(0)|, |off_re(width-1)|), mi = max(|off_im(0)|, |off_im(height-1)|), D = sqrt(mr*mr + mi*mi)
 *     (an axis of 0 pixels contributes off(0) alone).
 *   The table of an orbit X with last index `last` is a function of X's stored f64 entries, D, b0 and bits.  It is empty when
 *   last < 2.
 *     Level 0 has n_0 = last - 1 entries; entry j belongs to m = j + 1:
 *       A = (X_m.re + X_m.re, X_m.im + X_m.im), B = (b0, 0), r = eps * sqrt(A.re*A.re + A.im*A.im).
 *     Level k+1 has n_{k+1} = floor(n_k / 2) entries, built while n_k >= 2; entry j merges x = entry 2j (the first) with
 *     y = entry 2j+1 of level k:
 *       A = (fma(Ay.re, Ax.re, -(Ay.im*Ax.im)), fma(Ay.re, Ax.im, Ay.im*Ax.re))
 *       B = (fma(Ay.re, Bx.re, -(Ay.im*Bx.im)) + By.re, fma(Ay.re, Bx.im, Ay.im*Bx.re) + By.im)
 *       q = (ry - sqrt(Bx.re*Bx.re + Bx.im*Bx.im) * D) / sqrt(Ax.re*Ax.re + Ax.im*Ax.im); if !(q > 0) then q = 0 (NaN too)
 *       r = rx < q ? rx : q.
 *     Every entry stores r2 = r*r.  An entry with r2 == 0 is never applied and its A and B are unspecified (they may have
 *     overflowed).  r is non-increasing in the level for a fixed first step (r <= rx).
 *     Why A is finite where r2 > 0.  Invariant: r |A| < 2^-19 for every entry.  Level 0: an entry that does not end its
 *     orbit has re*re + im*im <= 4 and the last entry is no level-0 entry (n_0 = last - 1), so |A| <= 4 (1 + 2^-51) and
 *     r |A| = eps |A|^2 <= 16 eps (1 + 2^-49) <= 2^-20 (1 + 2^-49).  Merge: the subtraction only lowers ry and the division
 *     rounds once, so r <= q <= (ry / |Ax|)(1 + 2^-51), and |A| <= |Ay| |Ax| (1 + 2^-50); hence r |A| <= ry |Ay| (1 + 2^-49),
 *     y's own bound, and over at most 24 levels the factors stay below 1 + 2^-44.  r2 > 0 needs r > 2^-538, so such an entry
 *     has |A| < 2^519: the product that A is did not overflow, given finite factors.  Ax is finite: rx >= r, so x is such an
 *     entry itself.  Ay is finite by the same bound whenever ry*ry > 0.  What is left is 0 < ry < 2^-537 beside r > 2^-538,
 *     that is |Ax| < 1: only if moreover |Ay| > 2^1024, hence |Ax| < 2^-505 — an orbit entry within 2^-506 of the critical
 *     point followed, inside one block, by a stretch whose derivative passes 2^1024 — A is non-finite beside r2 > 0.  Then
 *     A is still what this IEEE sequence gives, so the definition stays exact; |B| D <= ry bounds B the same way.
 *   Pixel loop.  State as PT's, plus the table T of the orbit being followed: X's, and after a Julia rebase K's.  While
 *   i < iterations:
 *     1. d2 = dz.re*dz.re + dz.im*dz.im.  If m >= 1 let j = m - 1; K is the largest k >= 1 with j % 2^k == 0, (j >> k) < n_k,
 *        i + 2^k <= iterations and d2 < r2 of entry j >> k of level k.  All four are monotone in k, so any search order
 *        finds the same K.  There is no K when m == 0, when the table is empty, or when level 1 fails.
 *     2. No K: one plain PT step, exactly PT's — the only way a single iteration is taken (level 0 exists only to build the
 *        levels above it).  K found, with (A, B) = entry j >> K of level K:
 *          dz'.re = fma(A.re, dz.re, fma(-A.im, dz.im, fma(B.re, dc.re, -(B.im*dc.im))))
 *          dz'.im = fma(A.re, dz.im, fma(A.im, dz.re, fma(B.re, dc.im, B.im*dc.re)))
 *          m += 2^K, i += 2^K, z = X_m + dz' per axis (m <= last always: 1 + ((j >> K) + 1) 2^K <= 1 + n_0).
 *     3. In both cases test as PT does: dist = z.re*z.re + z.im*z.im; dist > limit*limit escapes with (z, i - 1), i already
 *        advanced; otherwise rebase on PT's condition.
 *     4. Exhaustion gives (z, iterations).
 *   Escapes inside a skipped block are not looked for: that is part of the definition.  The radii keep z within a relative
 *   eps of a reference entry that has not escaped.
 * Domain: PT's, or WIDE PT's with a centre; bits 0 (= FR_BLA_DEFAULT_BITS) or 24 .. 53; iterations <= FR_PT_MAX_ITERATIONS,
 * which bounds the tables: on the device an orbit's table holds fewer than `last` entries of 40 B (Mandelbrot) or 24 B (Julia,
 * two orbits), beside the orbit's own 16 B per entry — at most 640 MiB (768 MiB for Julia's two) at the cap.  One device;
 * block-cyclic and multi-device renders do not take BLA-PT (supersampling does, through fr_render_rows_ss_pt(_device) with
 * FR_PT_ROAD_BLA, not through fr_render_rows_ss), nor do the resumable-state and extend calls: the
 * condition i + 2^k <= iterations makes a run at cap N no prefix of the run at cap M, so there is no state to continue, and
 * fr_escape_extend(_device) and fr_escape_extend_pt(_device) have no BLA form.
 *
 * SCALED PT (the fr_*_pt_scaled calls below): WIDE PT and BLA-PT past a scale of 2^440, down to just under 2^952.  The pixel
 * loops above work in absolute units, and past 2^440 the squares they compare (|dz|^2 in the rebase test, r2 and d2 in
 * BLA-PT) leave f64's normal range.  SCALED PT carries the pixel's offset as w = dz 2^e, e the exponent of the view's scale.
 * The reference orbits and their stop rule, "ended by escape", the escape test and the colour map on the f64 z are WIDE PT's,
 * word for word, and the orbit cache is shared: a scaled call and a wide call of the same view, words and cap serve each
 * other's orbit.  Every operation below is one correctly rounded f64 operation; fma is fused and nothing else is; sqrt is IEEE.
 *   Constants of a view: max(|scale.re|, |scale.im|) = f 2^e with 0.5 <= f < 1 (the e of F >= e + 64); S = 2^e, Sinv = 2^-e;
 *   sre = scale.re * Sinv and sim = scale.im * Sinv, both exact;
 *     woff_re = ((x / h) - ((w / h) / 2)) / sre, woff_im = ((y / h) - 0.5) / sim
 *   — PT's operations of off with the scaled divisor; off itself is never formed; wc = woff for Mandelbrot, 0 for Julia.
 *   Pixel state (X, m, z, w): m starts as in PT, w = woff, z = fma(w, Sinv, X_m) per axis.
 *   Step i = 0 .. iterations-1:
 *     t  = X_m + z
 *     w' = (fma(t.re, w.re, fma(-t.im, w.im, wc.re)), fma(t.re, w.im, fma(t.im, w.re, wc.im)))
 *     m  = m + 1;  z = fma(w', Sinv, X_m) per axis;  w = w'
 *     dist = z.re*z.re + z.im*z.im: dist > limit*limit -> escape with (z, i)
 *     Rebase test.  w is BIG when max(|w.re|, |w.im|) >= 2^500.  BIG: d = w * Sinv per axis and the test is
 *     dist < d.re*d.re + d.im*d.im.  Otherwise a = z * S per axis and the test is a.re*a.re + a.im*a.im < w.re*w.re + w.im*w.im;
 *     an infinite left side makes it false, which is intended and IEEE-defined.  Rebase on the test or on m == last of X, as
 *     PT does: w = z * S per axis, m = 0 (z unchanged), and Julia then follows K.
 *   Exhaustion: (z, iterations).
 *   With a table (bits >= 0) the loop is BLA-PT's on (w, wc): the table of an orbit has BLA-PT's A and B unchanged and one
 *   replacement, the entry's scaled radius R where BLA-PT has r:
 *     Level 0: R = (eps * S) * sqrt(A.re*A.re + A.im*A.im)                                            (eps * S is exact)
 *     Merge:   Q = (Ry - sqrt(Bx.re*Bx.re + Bx.im*Bx.im) * Dw) / sqrt(Ax.re*Ax.re + Ax.im*Ax.im); if !(Q > 0) then Q = 0;
 *              R = Rx < Q ? Rx : Q
 *     Dw = sqrt(mrw*mrw + miw*miw) with mrw = max(|woff_re(0)|, |woff_re(width-1)|), miw = max(|woff_im(0)|,
 *     |woff_im(height-1)|): D's expression on woff, over the WHOLE image.
 *     An entry STORES R itself, not its square, and stores 0 when R < 2^-53; a stored 0 is never applied.  (A merge reads
 *     the R of its two entries as computed, before that rule.)
 *     Why A is finite where R > 0 is stored.  BLA-PT's invariant reads R |A| < 2^(e-19) here (it scales with S), and a stored
 *     R is at least 2^-53, so |A| < 2^(e+34) <= 2^986: no product that A is has overflowed, given finite factors, and the
 *     factors are entries with Rx >= R and Ry >= R |Ax| (1 - 2^-50) > 0 by the same two roundings.  There is no footnote case:
 *     nothing here depends on a radius below 2^-53, let alone on a subnormal one.
 *   Level search: BLA-PT's four conditions with the fourth as (w.re*f)*(w.re*f) + (w.im*f)*(w.im*f) < (R*f)*(R*f), where
 *   f = Sinv when w is BIG and 1 otherwise — one multiplication per operand, and the same two-sided IEEE behaviour as the
 *   rebase test: (R*f)*(R*f) may be +inf (then the condition holds for every finite left side) or 0.
 *   The skip is BLA-PT's expression on (w, wc) with (A, B) of the entry, followed by m += 2^K, i += 2^K and
 *   z = fma(w', Sinv, X_m) per axis; the tests are the plain scaled loop's, with (z, i - 1) on escape.
 *   w stays finite: a w that is not rebased has |w Sinv|^2 <= dist <= limit^2, and one step multiplies |w| by at most
 *   |X_m + z| <= 2 + limit + ... and adds |wc| <= 2^e, so |w| stays below about (limit^2 + 2) 2^e <= (2^40 + 2) 2^952 <
 *   2^1023 with limit <= 2^20; a rebase sets |w| = |z| S <= limit 2^e.
 *   CLAIM: for every view in WIDE PT's domain with limit <= 2^20 in which no intermediate of the unscaled run is subnormal,
 *   the scaled calls give WIDE PT's z and iters bit for bit with bits = -1, and BLA-PT's z and iters with bits >= 0
 *   (multiplying by 2^e commutes with every rounding: w = dz 2^e, R = r 2^e, Dw = D 2^e, and each comparison is the unscaled
 *   one with both sides scaled by the same power of two).  The pass counts may differ only for a pixel with |w| < 2^-53:
 *   BLA-PT may apply to it an entry whose R is stored as 0 here.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): WIDE PT's, with a centre REQUIRED, and with
 * these changes: limit <= 2^20 (the default, 65536, is inside); min(|scale.re|, |scale.im|) >= 2^-32 max(|scale.re|,
 * |scale.im|); no 2^440 rule — what bounds the scale is F >= e + 64 with n <= 16, so e <= 952 and |scale| < 2^952; bits = -1
 * (no table: the plain scaled loop), 0 (= FR_BLA_DEFAULT_BITS) or 24 .. 53.  One device.  OUT OF SCOPE: block-cyclic and
 * multi-device renders do not take SCALED PT; supersampling takes it through fr_render_rows_ss_pt(_device) with
 * FR_PT_ROAD_SCALED, not through fr_render_rows_ss.  Its plain loop (bits = -1) has a resumable state and an extend
 * form, RESUMABLE SCALED PT below; its table form (bits >= 0) has neither, for BLA-PT's reason: the condition
 * i + 2^k <= iterations makes a run at cap N no prefix of the run at cap M.  A state written by the fr_*_pt_wide_state calls is
 * no input of the scaled extension: it holds dz where the scaled state holds w.
 *
 * RESUMABLE SCALED PT (fr_escape_rows_pt_scaled_state, fr_escape_extend_pt_scaled below): the state that lets a SCALED PT
 * view's cap be raised in place.  It is SCALED PT's plain loop (bits = -1) with ONE change, to the rebase condition: rebase on
 * the scaled rebase test, or when m == last of X AND X is ended by escape.  Both forms of the scaled rebase test (BIG and
 * not) stay as they are; "ended by escape" and "cut by the cap" are RESUMABLE PT's terms, applied to the stored f64 entries.
 *   The resumable state of a pixel after N steps is (z, w, m, onK).  Stored form, 40 bytes per pixel, in RESUMABLE PT's
 *   layout: z (2 doubles, as fr_escape_rows_pt_scaled gives it with bits = -1), iters (one uint32), w (2 doubles: the SCALED
 *   offset — this array holds w, not dz), m as uint32 whose bit 31 is set when a Julia pixel follows K (never for
 *   Mandelbrot).  An escaped pixel stores w = (0, 0), m = 0.  N = 0 stores the initial state (Mandelbrot: m = 1; Julia:
 *   m = 0; w = woff; z = fma(w, Sinv, X_m) per axis).
 *   CLAIM 1: for every N, z and iters of the state run equal SCALED PT's at cap N with bits = -1, bit for bit.
 *   CLAIM 2: continuing the state from N for M - N steps on the orbits of cap M gives the state run at cap M, bit for bit in
 *   all four arrays.
 *   Why: RESUMABLE PT's argument, word for word.  It uses only the bounds on m (after step i, m <= i + 2 for Mandelbrot or
 *   i + 1 for Julia on V, and m <= N - 1 on K after a rebase) and last = N + 1 (R) or N (V, K) of an orbit cut by the cap; the
 *   scaling touches neither.  So on a cut orbit m == last is met only at the final step i = N - 1, by a pixel that never
 *   rebased; there SCALED PT's rebase changes (w, m) and leaves z alone, which is invisible in its output and is the only
 *   event of the loop that depends on the cap.  The state rule leaves it out.
 *   CLAIM 3: for every view in WIDE PT's domain with limit <= 2^20 in which no intermediate of the unscaled run is subnormal,
 *   z, iters and m equal those of fr_escape_rows_pt_wide_state bit for bit, and w equals dz 2^e exactly (multiplication by
 *   a power of two commutes with every rounding).
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): SCALED PT's, with the centre REQUIRED; there
 * is no bits argument, the calls are the plain loop's; for the extension M >= N (M == N is a legal no-op that needs no
 * device, as y0 == y1 is); all four arrays, z and w 8-byte aligned, iters and m 4-byte aligned (y0 == y1 needs none). */
/*
 * DE (distance estimation; the fr_escape_rows_de, fr_distance_rows and fr_colour_de calls below): the orbit's derivative
 * carried beside the escape loop, the exterior distance estimate derived from it, and the colour map shaded by that distance.
 * DE is defined on two roads: FR_PRECISION_F64, and FR_PRECISION_PT with a dd centre (pos, pos_lo) or a wide centre (WIDE PT).
 * Every operation below is ONE correctly rounded f64 operation; fma is fused and nothing else is; sqrt is IEEE; log2 is the
 * software log2 the colour map uses (fr_log2 of csrc/fr_math.h).
 *   Derivative.  b0 = 1 for Mandelbrot (d/dc), 0 for Julia (d/dz0).  The derivative d accompanies `previous` and starts as
 *   (1, 0).  In step i the road's own step forms `next` from previous = z — F64: recursive(), calc/src/lib.rs:245-257, with
 *   its operation order; PT: PT's step on (X, m, z, dz) above, word for word, rebases included — and beside it, from the same z
 *   (the f64 position before the step; in PT the z the loop already holds):
 *     t  = (z.re + z.re, z.im + z.im)
 *     nd = (fma(t.re, d.re, fma(-t.im, d.im, b0)), fma(t.re, d.im, t.im * d.re))
 *   Escape returns (next, i, nd); otherwise d = nd; exhaustion returns (previous, iterations, d): `der` is always the
 *   derivative of the returned position, and iterations = 0 returns (start, 0, (1, 0)).  d may become +-inf or NaN: that is
 *   the IEEE result of this sequence and part of the definition (a NaN's sign and payload are not specified).  z and iters
 *   are the road's own, bit for bit (fr_escape_rows_device, fr_escape_rows_pt, fr_escape_rows_pt_wide).  An algorithm without
 *   orbits writes zeros into all three arrays.
 *   Distance, in pixels, per pixel:
 *     if iters == iterations: D = 0
 *     else n2  = z.re*z.re + z.im*z.im;  dn2 = d.re*d.re + d.im*d.im
 *          num = (sqrt(n2) * log2(n2)) * 0x1.62e42fefa39efp-2                            [|z| ln|z|]
 *          D   = (num / sqrt(dn2)) * ((double)height * min(|scale.re|, |scale.im|))      [the last factor: one product]
 *          if !(D > 0) D = 0            [NaN and negatives; +inf stays: d == 0, nothing is near]
 *   This is b = |z| ln|z| / |z'|; close to the set the true distance lies in (b/2, 2b).  dn2 = +inf (|d| >= 2^512, or d
 *   itself inf / NaN) gives D = 0, which inside the domain below happens only to pixels far below one pixel from the set,
 *   where 0 is what should be drawn (DESIGN.md 3.20 carries the bound: b < height * min|scale| * 2^-465 pixels there).
 *   Shading.  fr_colour_de_rows applies the colour map exactly as fr_colour_rows_device does; then, for a pixel with
 *   iters < iterations, thickness > 0 and s = D / thickness < 1, every colour byte becomes (uint8_t)((double)byte * s),
 *   truncated.  Alpha stays 255.  Capped pixels are never shaded: their inside colour is the reference's.  thickness == 0
 *   gives fr_colour_rows_device's bytes exactly.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): the road's own domain; limit <= 2^20;
 * thickness finite and in [0, 2^20]; F64 takes no pos_lo; PT with a wide centre keeps WIDE PT's |scale| <= 2^440.
 * Out of scope of these calls, refused by name: FR_PRECISION_F32, FR_PRECISION_DD, BLA-PT (these calls know no table: DE ON BLA-PT
 * below has calls of its own) and SCALED PT; block-cyclic and multi-device renders; fr_pixel.  Supersampling is SUPERSAMPLED DE
 * below (fr_render_rows_ss_de, fr_colour_de_rows_ss_device), not these calls.  AFTER fr_escape_extend* ON (z, iters) ALONE,
 * A der ARRAY IS STALE: it is the derivative at the old cap's position, and those calls do not know of it.  The calls that
 * continue all arrays are fr_escape_extend_de(_device) on the F64 road and fr_escape_extend_de_pt(_device) on PT (RESUMABLE DE
 * below); a PT view whose cap will be raised is rendered with fr_escape_rows_de_pt_state, not fr_escape_rows_de. */
/*
 * RESUMABLE DE (fr_escape_extend_de, fr_escape_rows_de_pt_state, fr_escape_extend_de_pt below): the state that lets a DE view's
 * cap be raised in place, derivative included.  The derivative is part of the loop's state like everything else.
 *   F64.  The stored (z, iters, der) of fr_escape_rows_de IS the resumable state: exhaustion returns (previous, iterations, d),
 *   and c is a function of the pixel, recomputed by the render's own coordinate code.  Continuing a pixel with iters == N for
 *   M - N steps of DE's F64 step from (previous, d) is the loop at cap M, bit for bit in all three arrays.
 *   PT (dd or wide centre).  The resumable state of a pixel after N steps is (z, dz, m, onK, d), stored as (z, iters, dz, m,
 *   der), 56 bytes per pixel, in RESUMABLE PT's form (bit 31 of m: a Julia pixel on K).  It is RESUMABLE PT's state run — PT's
 *   step sequence with the rebase rule "dist < |dz|^2, or m == last of an orbit ENDED BY ESCAPE" — with DE's derivative beside
 *   it: in every step, from the z before the step,
 *     t  = (z.re + z.re, z.im + z.im)
 *     nd = (fma(t.re, d.re, fma(-t.im, d.im, b0)), fma(t.re, d.im, t.im * d.re)),     d0 = (1, 0).
 *   Escape stores (next, i, dz = (0, 0), m = 0, nd); exhaustion stores (z, N, dz, m | onK << 31, d).  N = 0 stores RESUMABLE PT's
 *   initial state with der = (1, 0).  An algorithm without orbits writes zeros into all five arrays.
 *   CLAIM 1: for every N, z, iters and der of the PT state run equal fr_escape_rows_de's (PT) bit for bit, and dz and m equal
 *   fr_escape_rows_pt_state's.
 *   Why: the derivative reads only z.  RESUMABLE PT's claim says the z sequence of the state run is PT's; the one cap-dependent
 *   rebase, which the state rule leaves out, changes (dz, m) and never z.
 *   CLAIM 2: continuing the state from N for M - N steps on the orbits of cap M gives the state run at cap M, bit for bit in
 *   all five arrays (a NaN in der is any NaN, as in DE).
 *   Why: RESUMABLE PT's argument for (z, iters, dz, m), plus "d is a function of the z sequence": d after step i is determined
 *   by d0 and z_0 .. z_i, which a state run to N and a state run to M share up to N.
 * Domain: DE's, unchanged (limit <= 2^20; PT's domain with a dd centre, WIDE PT's |scale| <= 2^440 with a wide one); M >= N.
 * The overflow bound of DE is about the step that is returned and does not depend on where a run was
 * interrupted: a continued derivative takes the same values, overflow included, as the uninterrupted one.
 * DE on SCALED PT stays out of scope; DE ON BLA-PT (below) has no state: neither is resumable with a derivative.  That is the
 * scope of THESE calls; RESUMABLE SCALED DE below has calls of its own for the plain scaled loop. */
/*
 * DE ON BLA-PT (fr_escape_rows_de_pt_bla(_device) below): the derivative carried through the table's skips.  It is BLA-PT's
 * definition above word for word, with a dd centre (pos, pos_lo) or a wide centre (WIDE PT's domain) — the orbits, the table with
 * D, bits and b0, the level search, the plain step, the skip, the escape test, the rebase rule, and (z, i - 1) on escape after
 * a skip — with the derivative d carried beside it, d0 = (1, 0).  Every operation is ONE correctly rounded f64 operation; fma
 * is fused and nothing else is.  In one pass of BLA-PT's loop:
 *   Plain step (no level K found): DE's step, from the z before the step:
 *     t  = (z.re + z.re, z.im + z.im)
 *     nd = (fma(t.re, d.re, fma(-t.im, d.im, b0)), fma(t.re, d.im, t.im * d.re))
 *   Skip with the entry (A, B) of level K: b = B for Mandelbrot; b = (+0, +0) for Julia (its device table stores no B, and
 *   b0 = 0 there);
 *     nd.re = fma(A.re, d.re, fma(-A.im, d.im, b.re))
 *     nd.im = fma(A.re, d.im, fma( A.im, d.re, b.im))
 *   Escape returns (z, i - 1, nd); otherwise d = nd; exhaustion returns (z, iterations, d).  A rebase never touches d.
 *   iterations = 0 returns (start, 0, (1, 0)).  An algorithm without orbits writes zeros into all three arrays.  d may become
 *   +-inf or NaN: that is the IEEE result of this sequence and part of the definition, as in DE (a NaN is any NaN).
 *   Why the skip is the derivative: over a block of 2^K steps d' = prod(2 z_k) d + b0 sum(...), and the table's level-0 entry
 *   A = 2 X_m, B = (b0, 0) with its merge A = Ay Ax, B = Ay Bx + By is that recurrence with X_k in place of z_k.  A skip is
 *   applied only while |dz| < r = eps |2X|, so every factor is off by a relative |dz_k| / |X_k| < 2 eps.  No table data is
 *   added and no table is rebuilt: the calls share the context's table with the fr_*_pt_bla calls of the same view and bits.
 *   CLAIM 1: z and iters are fr_escape_rows_pt_bla's, bit for bit: the derivative only reads.
 *   CLAIM 2: on a view where no pass skips, all three arrays are fr_escape_rows_de's (FR_PRECISION_PT), bit for bit.
 *   DE's overflow bound is about the returned step's derivative and carries over unchanged.  BLA-PT's invariant
 *   keeps A finite where r2 > 0; its stated footnote case gives a non-finite d, hence D = 0.
 *   The distance and the shading are DE's own, unchanged: fr_distance_rows(_device) and fr_colour_de_rows_device /
 *   fr_colour_de_rgb8 run over this call's (z, iters, der).  Measured accuracy against DE on plain PT: DESIGN.md 3.22.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): BLA-PT's, dd or wide centre (with a wide
 * centre |scale| <= 2^440); DE's limit <= 2^20; bits 0 (FR_BLA_DEFAULT_BITS) or 24 .. 53; all three arrays, z and der 8-byte
 * aligned, iters 4-byte aligned; y0 == y1 is a no-op that needs no device and no array.
 * Out of scope: SCALED PT (past 2^440 the derivative itself leaves the range in which dn2 = |d|^2 is finite: that road needs a
 * scaled derivative and an overflow argument of its own); a resumable state or an extend form (BLA-PT has none: i + 2^k <=
 * iterations makes a run at cap N no prefix of the run at cap M); multi-device and block-cyclic renders; the command line
 * (--distance-shade with --bla stays refused).  Supersampling is SUPERSAMPLED DE below, with FR_PT_ROAD_BLA. */
/*
 * DE ON SCALED PT (fr_escape_rows_de_pt_scaled(_device) and fr_de_scaled_view below): distance estimation past a scale of 2^440,
 * with its own calls; the DE calls above and SUPERSAMPLED DE below keep refusing SCALED PT.  At a pixel D pixels from the set
 * |d| is about |z| ln|z| * height * |scale| / D, of the order 2^e and above, so dn2 = |d|^2 leaves f64 from e = 512.  The
 * road carries a SCALED derivative u = d 2^-e instead, as it carries w = dz 2^e for the offset.
 * It is SCALED PT's definition above word for word, in both forms (bits = -1, the plain scaled loop, and bits >= 0, the table) —
 * the orbits, S, Sinv, sre, sim and woff; the pixel state, the step and the BIG / not-BIG rebase test; the table with R and Dw,
 * the level search, the skip and the escape test — and beside it runs the scaled derivative u.  Every operation is ONE correctly
 * rounded f64 operation; fma is fused and nothing else is.
 *   u0 = (Sinv, 0).  bs0 = Sinv for Mandelbrot and 0 for Julia.
 *   Plain step, from the z the loop holds before the step:
 *     t  = (z.re + z.re, z.im + z.im)
 *     nu = (fma(t.re, u.re, fma(-t.im, u.im, bs0)), fma(t.re, u.im, t.im * u.re))
 *   Skip with the entry (A, B) of level K: b = (B.re * Sinv, B.im * Sinv) for Mandelbrot, one multiplication each;
 *   b = (+0, +0) for Julia;
 *     nu = (fma(A.re, u.re, fma(-A.im, u.im, b.re)), fma(A.re, u.im, fma(A.im, u.re, b.im)))
 *   Escape returns (z, index, nu), the index being i in the plain loop and i - 1 after a pass of the table form; otherwise
 *   u = nu.  Exhaustion returns (z, iterations, u).  A rebase never touches u.  iterations = 0 returns (start, 0, (Sinv, 0)).
 *   An algorithm without orbits writes zeros.  u may become +-inf or NaN, as in DE (a NaN is any NaN).  The stored der array
 *   holds u: the derivative with respect to the view's SCALED coordinate.
 *   THE SCALED VIEW: cfg_v is cfg with scale = (sre, sim) = (scale.re * Sinv, scale.im * Sinv), both products exact, every other
 *   field unchanged (fr_de_scaled_view writes it).  The distance and the shading are DE's own calls, run on cfg_v:
 *   fr_distance_rows(_device), fr_colour_de_rows_device, fr_colour_de_rgb8, and fr_colour_de_rows_ss_device for a kept view.  Of
 *   the view they read only height, scale, iterations and the colour fields, so
 *     D = (num / sqrt(u.re*u.re + u.im*u.im)) * ((double)height * min(|sre|, |sim|))
 *   — d = u 2^e and scale = (sre, sim) 2^e: the factor 2^e cancels in D.  No distance or colour kernel is added or changed.
 *   CLAIM 1: z and iters are fr_escape_rows_pt_scaled's for the same bits, bit for bit: the derivative only reads.
 *   CLAIM 2: in the common domain (WIDE PT's: |scale| <= 2^440, limit <= 2^20), and where no intermediate of either run is
 *   subnormal or overflows, u = d 2^-e exactly, d from fr_escape_rows_de_pt_wide for bits = -1 or from fr_escape_rows_de_pt_bla
 *   with the wide centre for bits >= 0 (the latter with SCALED PT's own caveat about a pixel with |w| < 2^-53), and D on cfg_v
 *   equals D of DE on cfg, bit for bit.  The reason: (q 2^e) (p 2^-e) rounds as q p does — every product in the u chain is the
 *   product of the d chain times 2^-e, bs0 = b0 2^-e and B Sinv = B 2^-e are exact, and in D the scale's 2^e cancels the same way.
 *   CLAIM 3, the range (DESIGN.md 3.24 writes the argument out).  Overflow: un2 = u.re*u.re + u.im*u.im = +inf needs a component
 *   of u near 2^512, which gives D = 0 where the true distance is below about height * 2^-465 pixels: DE's bound carried over,
 *   since pixels_v = height * min(|sre|, |sim|) <= height.  Underflow: un2 underflows only for |u| < 2^-511; then D exceeds every
 *   admissible thickness (<= 2^20) or is +inf, such a pixel is never shaded and never should be, and ITS REPORTED DISTANCE IS
 *   NOT ACCURATE THERE.  Components: a single component of u may go subnormal beside a large one (|component of d| < 2^(e-1022));
 *   its square is below 2^-2044 of the other's and does not move un2, hence not D.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): SCALED PT's, with the centre REQUIRED; its
 * limit <= 2^20 is DE's too; bits -1, 0 (FR_BLA_DEFAULT_BITS) or 24 .. 53; all three arrays, z and der 8-byte aligned, iters
 * 4-byte aligned; y0 == y1 is a no-op that needs no device and no array.
 * Out of scope: a resumable state or an extend form for scaled DE; supersampling (fr_render_rows_ss_de keeps refusing
 * FR_PT_ROAD_SCALED; a kept scaled view is filtered by fr_colour_de_rows_ss_device on cfg_v); the command line; the Rust shim;
 * multi-device and block-cyclic renders.  The first two are out of scope of THESE calls; RESUMABLE SCALED DE and SUPERSAMPLED
 * SCALED DE below have calls of their own. */
/*
 * RESUMABLE SCALED DE (fr_escape_rows_de_pt_scaled_state, fr_escape_extend_de_pt_scaled below): the state that lets a DE view past
 * a scale of 2^440 have its cap raised in place, scaled derivative included.  The state of a pixel after N steps is
 * (z, w, m, onK, u).  It is RESUMABLE SCALED PT's state run, word for word — the plain scaled loop, bits = -1; the rebase rule
 * "the scaled rebase test, or m == last of an orbit ENDED BY ESCAPE"; both forms of the test, BIG and not BIG — with DE ON SCALED
 * PT's plain-step derivative beside it: u0 = (Sinv, 0), bs0 = Sinv for Mandelbrot and 0 for Julia, and in every step, from the
 * z the loop holds before the step,
 *     t  = (z.re + z.re, z.im + z.im)
 *     nu = (fma(t.re, u.re, fma(-t.im, u.im, bs0)), fma(t.re, u.im, t.im * u.re)).
 * A rebase never touches u.  Every operation is ONE correctly rounded f64 operation; fma is fused and nothing else is.
 *   Stored form, 56 bytes per pixel: the arrays (z, iters, w, m, der) in RESUMABLE SCALED PT's layout (w holds the SCALED offset,
 *   bit 31 of m: a Julia pixel on K) with der = u, 2 doubles, beside them.  Escape stores (next, i, w = (0, 0), m = 0, nu);
 *   exhaustion stores (z, N, w, m | onK << 31, u).  N = 0 stores RESUMABLE SCALED PT's initial state with der = (Sinv, 0).  An
 *   algorithm without orbits writes zeros into all five arrays.
 *   CLAIM 1: for every N, z, iters and der equal fr_escape_rows_de_pt_scaled's with bits = -1, and w and m equal
 *   fr_escape_rows_pt_scaled_state's, bit for bit.
 *   Why: u reads only z.  RESUMABLE SCALED PT's claim 1 says the z sequence of the state run is SCALED PT's; the one
 *   cap-dependent rebase, which the state rule leaves out, changes (w, m) and never z, hence never u.  (z, iters, w, m) are
 *   computed by RESUMABLE SCALED PT's operations, which u does not enter.
 *   CLAIM 2: continuing the state from N for M - N steps on the orbits of cap M gives the state run at cap M, bit for bit in all
 *   five arrays (a NaN in der is any NaN, as in DE).
 *   Why: RESUMABLE SCALED PT's claim 2 for (z, iters, w, m), plus "u is a function of the z sequence": u after step i is
 *   determined by u0 and z_0 .. z_i, which a state run to N and a state run to M share up to N.
 *   CLAIM 3: in WIDE PT's domain with limit <= 2^20, where no intermediate of either run is subnormal or overflows, z, iters
 *   and m equal fr_escape_rows_de_pt_state's with the wide centre, w = dz 2^e, and der 2^e is its der, all exactly.
 *   Why: RESUMABLE SCALED PT's claim 3 for (z, iters, w, m) and DE ON SCALED PT's claim 2 for u: multiplication by a power of two
 *   commutes with every rounding, and u reads only z, which is the same in both runs.
 *   The range argument of DE ON SCALED PT (its CLAIM 3) is about the returned step's u and does not depend on
 *   where a run was interrupted: a continued u takes the same values, overflow and underflow included, as the uninterrupted one.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): SCALED PT's, with the centre REQUIRED (DE's
 * limit <= 2^20 is already SCALED PT's); there is no bits argument, the calls are the plain loop's; for the extension M >= N
 * (M == N is a legal no-op that needs no device, as y0 == y1 is); all five arrays non-NULL, z, w and der 8-byte aligned, iters
 * and m 4-byte aligned (y0 == y1 needs none).  The table form (bits >= 0) has no state, for BLA-PT's reason: the condition
 * i + 2^k <= iterations makes a run at cap N no prefix of the run at cap M. */
/*
 * SUPERSAMPLED DE (fr_render_rows_ss_de, fr_colour_de_rows_ss_device below): distance estimation and supersampling at once —
 * filaments thinner than a pixel stay visible AND the borders are anti-aliased.  DEFINITION, for supersample = s,
 * 1 <= s <= FR_SS_MAX, and a thickness T in OUTPUT pixels:
 *   cfg_s = cfg with width * s and height * s, every other field unchanged;
 *   (z, iters, der) = the road's DE render of cfg_s, bit for bit what the existing call writes:
 *             FR_PRECISION_F64                       fr_escape_rows_de(cfg_s, FR_PRECISION_F64, NULL, ...);
 *             FR_PRECISION_PT, FR_PT_ROAD_PLAIN      fr_escape_rows_de(cfg_s, FR_PRECISION_PT, pos_lo, ...), or with a wide
 *                                                    centre fr_escape_rows_de_pt_wide(cfg_s, centre, ...);
 *             FR_PRECISION_PT, FR_PT_ROAD_BLA        fr_escape_rows_de_pt_bla(cfg_s, pos_lo, centre, bits, ...); its D is taken
 *                                                    over the whole image of cfg_s, as the supersampled deep roads define;
 *   Ts    = T * (double)s, one f64 product;
 *   H     = the bytes of fr_colour_de_rows_device(cfg_s, z, iters, der, n, Ts, 3): the distance is in SAMPLE pixels — its last
 *           factor is (double)(s * height) * min(|scale.re|, |scale.im|) — and so is Ts, hence the line stays T output pixels
 *           wide whatever s is;
 *   out(X, Y, c) = (sum over j < s, i < s of H(s*X + i, s*Y + j, c) + floor(s*s / 2)) / (s*s)
 *           in integer arithmetic, truncating; with 4 channels alpha is 255: the box filter of "supersampled rendering".
 * s = 1 is the road's DE render followed by fr_colour_de_rows_device(cfg, ..., T, channels), byte for byte.  T = 0 gives the
 * bytes of the unshaded supersampled render of the same road (fr_render_rows_ss / fr_render_rows_ss_pt).  An algorithm without
 * orbits gives black.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): s in 1 .. FR_SS_MAX; s * width and s * height
 * fit in 32 bits; the road's own DE domain ON cfg_s, checked by the code the plain calls run; T finite with 0 <= T * s <= 2^20
 * (Ts is then inside fr_colour_de_rows_device's own domain: the definition is literally a composition of existing calls);
 * channels 3 or 4.  Refused by name: FR_PRECISION_F32 and FR_PRECISION_DD (DE's scope message), FR_PT_ROAD_SCALED (DE on SCALED
 * PT stays out of scope).  One device.  The command line stays as it is: --distance-shade beside --supersample above 1 or
 * --bla is refused there.  FR_PT_ROAD_SCALED is out of scope of THESE calls; SUPERSAMPLED SCALED DE below has calls of its own.
 */
/*
 * SUPERSAMPLED SCALED DE (fr_render_rows_ss_de_pt_scaled(_device) below): SUPERSAMPLED DE past a scale of 2^440, on DE ON SCALED
 * PT's road, with its own calls; fr_render_rows_ss_de keeps refusing FR_PT_ROAD_SCALED.  DEFINITION, for supersample = s,
 * 1 <= s <= FR_SS_MAX, and a thickness T in OUTPUT pixels:
 *   cfg_s  = cfg with width * s and height * s, every other field unchanged;
 *   (z, iters, u) = fr_escape_rows_de_pt_scaled(cfg_s, centre, bits, ...), bit for bit; bits is -1, 0 or 24 .. 53; its Dw is
 *            taken over the whole image of cfg_s, as the supersampled deep roads define;
 *   cfg_sv = fr_de_scaled_view(cfg_s): cfg_s with scale = (sre, sim);
 *   Ts     = T * (double)s, one f64 product;
 *   H      = the bytes of fr_colour_de_rows_device(cfg_sv, z, iters, u, n, Ts, 3): the distance is in SAMPLE pixels, its last
 *            factor (double)(s * height) * min(|sre|, |sim|), one product;
 *   out    = SUPERSAMPLED DE's integer box filter of H:
 *            out(X, Y, c) = (sum over j < s, i < s of H(s*X + i, s*Y + j, c) + floor(s*s / 2)) / (s*s), truncating; with 4
 *            channels alpha is 255.
 * s = 1 is fr_escape_rows_de_pt_scaled followed by fr_colour_de_rows_device(cfg_v, ..., T, channels), byte for byte.  T = 0 gives
 * the bytes of fr_render_rows_ss_pt(..., FR_PT_ROAD_SCALED, bits, s).  An algorithm without orbits gives black.  A KEPT
 * anti-aliased scaled view — (z, iters, w, m, u) of cfg_s, written by fr_escape_rows_de_pt_scaled_state_device and kept current
 * by fr_escape_extend_de_pt_scaled_device — recoloured by fr_colour_de_rows_ss_device on cfg_v gives the same bytes as this
 * render with bits = -1 at the view's cap.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): s in 1 .. FR_SS_MAX; s * width and s * height
 * fit in 32 bits; DE ON SCALED PT's domain ON cfg_s, checked by the code the plain calls run (centre required; bits -1, 0 or
 * 24 .. 53); T finite with 0 <= T * s <= 2^20; channels 3 or 4; the buffer and workspace rules of fr_render_rows_ss_de_device
 * (fr_ss_de_workspace_bytes plans the workspace, 36 bytes per sample).  No colour or filter kernel is added or changed.
 * Taking all s*s samples only at edge pixels and near the set is out of scope of THESE calls; ADAPTIVE SUPERSAMPLED SCALED DE below
 * has calls of its own.
 */
#define FR_BLA_DEFAULT_BITS 40
#define FR_PT_MAX_ITERATIONS (1u << 24)
#define FR_WIDE_MAX_WORDS 16
typedef enum fr_precision {
    FR_PRECISION_F64 = 0,
    FR_PRECISION_F32 = 1,
    FR_PRECISION_DD = 2,
    FR_PRECISION_PT = 3
} fr_precision;

/* ---- lifetime ---------------------------------------------------------------------------- */

/* Select the HIP device the single-device entry points render on (-1 = keep the current one /
 * device 0) and create the library's state.  Optional: compute calls auto-initialise on device 0.
 * Switching to another device waits for every call in flight and frees the state on the old one. */
int fr_init(int device);
/* Release streams and scratch memory.  Safe to call twice; the library can be re-initialised. */
int fr_shutdown(void);
int fr_device_count(int *count);
/* gfx architecture name of the active device, e.g. "gfx950:sramecc+:xnack-" */
int fr_device_name(char *buf, size_t buf_len);
const char *fr_last_error(void);
int fr_abi_version(void);
/* SHA-256 prefix over the sources and flags this binary was built from (fractal-renderer_amd/build.py) */
const char *fr_build_id(void);

/* Config::new(algo) — calc/src/lib.rs:39-69 */
void fr_config_new(fr_config *cfg, uint32_t algo);

/* ---- get_image — src/lib.rs:253-270 ------------------------------------------------------- */

/* Whole image into a HOST buffer of at least 3*width*height bytes (f64 arithmetic).
 * Replaces `get_image(config)` for Algo::Mandelbrot | Algo::Julia. */
int fr_render_rgb8(const fr_config *cfg, uint8_t *out, size_t out_len);

/* Rows [y0, y1) of the image into a HOST buffer of at least 3*width*(y1-y0) bytes: the unit the
 * reference's rayon loop parallelises over (src/lib.rs:256-264).  y0 == y1 is legal (no-op). */
int fr_render_rows_rgb8(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, uint8_t *out,
                        size_t out_len);

/* Same, into DEVICE memory, asynchronously on `hip_stream` (a hipStream_t, NULL = the null
 * stream; STREAM ORDER above is the contract, here and for every call below that takes a stream).
 * For callers that keep the image in HBM (multi-GPU gather, GUI upload). */
int fr_render_rows_rgb8_device(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1,
                               void *d_out, size_t out_len, void *hip_stream);

/* The same rows as RGBA8 (bytes r,g,b,255; 4*width*(y1-y0) bytes; device pointer 4-byte aligned): what
 * the reference's GUI converts the Vec<RGB> to on the CPU before uploading it (src/gui.rs:71-72). */
int fr_render_rows_rgba8(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, uint8_t *out,
                         size_t out_len);
int fr_render_rows_rgba8_device(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, void *d_out,
                                size_t out_len, void *hip_stream);

/* Row-block-cyclic share of the image for multi-GPU rendering: blocks of `block_rows` rows,
 * this call renders blocks first_block, first_block + block_stride, ... and packs them
 * contiguously into d_out (device memory).  *rows_written (may be NULL) receives the number of
 * rows produced.  fr_block_cyclic_rows() returns that count without rendering. */
int fr_render_block_cyclic_rgb8_device(const fr_config *cfg, int precision, uint32_t block_rows,
                                       uint32_t first_block, uint32_t block_stride, void *d_out,
                                       size_t out_len, void *hip_stream, uint64_t *rows_written);
/* The same with two refinements used by the pipelined multi-GPU gather: at most `max_blocks` blocks
 * (0 = all), and `dest_is_image` != 0 to write every row at its place in the WHOLE image (d_out is
 * then the image base, out_len >= 3*width*height, block_rows % 8 == 0) instead of packing. */
int fr_render_block_cyclic_range_rgb8_device(const fr_config *cfg, int precision, uint32_t block_rows,
                                             uint32_t first_block, uint32_t block_stride, uint32_t max_blocks,
                                             int dest_is_image, void *d_out, size_t out_len, void *hip_stream,
                                             uint64_t *rows_written);

/* Same share into a HOST buffer (packed blocks, 3*width*rows bytes). */
int fr_render_block_cyclic_rgb8(const fr_config *cfg, int precision, uint32_t block_rows, uint32_t first_block,
                                uint32_t block_stride, uint8_t *out, size_t out_len, uint64_t *rows_written);
uint64_t fr_block_cyclic_rows(uint32_t height, uint32_t block_rows, uint32_t first_block,
                              uint32_t block_stride);

/* ---- per-call implementation selectors ------------------------------------------------------- */

/* Everything the fr_set_* calls below select process-wide, as an argument of ONE call, so that two
 * threads (the GUI's render and screenshot threads, src/gui.rs:56-60, 322-326) never share a knob.
 * None of them changes a single output byte.  Fill with fr_render_opts_init() (the process
 * defaults), change what you need, pass to an *_opts entry point; NULL means "the defaults". */
typedef struct fr_render_opts {
    uint32_t size;          /* sizeof(fr_render_opts): lets the struct grow without an ABI break */
    int32_t tile;           /* see fr_set_tile */
    int32_t loop_mode;      /* see fr_set_loop_mode */
    int32_t palette;        /* see fr_set_palette */
    int32_t cycle_shortcut; /* see fr_set_cycle_shortcut */
    int32_t refill_minrun;  /* see fr_set_refill_policy */
    int32_t refill_quit16;
    int32_t colour_filter;  /* see fr_set_colour_filter */
} fr_render_opts;
void fr_render_opts_init(fr_render_opts *opts);

int fr_render_rows_rgb8_device_opts(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, void *d_out,
                                    size_t out_len, void *hip_stream, const fr_render_opts *opts);
int fr_render_rows_rgba8_device_opts(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, void *d_out,
                                     size_t out_len, void *hip_stream, const fr_render_opts *opts);
int fr_render_rows_rgb8_opts(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, uint8_t *out,
                             size_t out_len, const fr_render_opts *opts);
int fr_render_block_cyclic_range_rgb8_device_opts(const fr_config *cfg, int precision, uint32_t block_rows,
                                                  uint32_t first_block, uint32_t block_stride, uint32_t max_blocks,
                                                  int dest_is_image, void *d_out, size_t out_len, void *hip_stream,
                                                  uint64_t *rows_written, const fr_render_opts *opts);

/* ---- get_image across several GPUs from ONE process ---------------------------------------- */

/* The reference is one process calling get_image once (src/main.rs:16, src/lib.rs:253); its rayon
 * loop spreads the rows over every core (src/lib.rs:256-258).  The counterpart here spreads row
 * blocks over every device of a set: block b (block_rows rows) is rendered by device b % n — the
 * set's interior sits in the middle rows of the default view, so contiguous bands would be badly
 * unbalanced — by one host thread and one set of streams per device.
 *
 * fr_init_devices: `devices` lists HIP device indices; an index may repeat ("logical devices" that
 * share a GPU: how a one-GPU box exercises the whole path).  Replaces any earlier set.  n <= 16. */
int fr_init_devices(const int *devices, int n);
int fr_multi_device_count(int *count);

/* Whole image into the caller's HOST buffer (>= 3*width*height bytes): every device DMAs each of its
 * finished row blocks straight to the block's final place over its own PCIe link while it renders
 * the next ones.  This is what a multi-GPU get_image costs its caller.  block_rows = 0: default (256). */
int fr_render_rgb8_multi(const fr_config *cfg, int precision, uint32_t block_rows, uint8_t *out, size_t out_len);

/* Whole image gathered into DEVICE memory of the set's first device (d_out, >= 3*width*height bytes,
 * allocated by the caller on that device): the first device renders its blocks in place, the others
 * send each finished block to its place over xGMI while they render the next ones —
 *   FR_GATHER_PEER_COPY  peer-to-peer DMA (hipMemcpyPeerAsync), works for repeated device indices too;
 *   FR_GATHER_RCCL       grouped ncclSend / ncclRecv on a communicator from ncclCommInitAll
 *                        (librccl is loaded on first use; needs distinct devices). */
/* The call renders on streams of the library's own and returns when the image is complete: work the CALLER has queued on
 * d_out on a stream of its own (a fill, an earlier reader) must have finished before the call. */
typedef enum fr_gather { FR_GATHER_PEER_COPY = 0, FR_GATHER_RCCL = 1 } fr_gather;
int fr_render_rgb8_multi_device(const fr_config *cfg, int precision, uint32_t block_rows, int gather, void *d_out,
                                size_t out_len);

/* Who renders the sink's row blocks.  The set's first device is both a renderer and the sink of the gather; by default it
 * renders all of its blocks (plain cyclic dealing, q = 1).  q = 2 / 4: it keeps every 2nd / 4th of them and the rest are dealt
 * round-robin to the other devices; q = 0: it renders nothing and only receives.  Same bytes; a tuning knob for the first
 * real multi-GPU run (bench.py --root-share, which prints where every device's time went).  Process-wide. */
int fr_set_multi_root_share(int q);

/* Timing of the calling thread's last multi-device render: per device, the time its render kernels
 * took (HIP events, summed over its chunks) and the host-side wall time of the whole call. */
#define FR_MAX_DEVICES 16
typedef struct fr_multi_stats {
    uint32_t n_devices;
    uint32_t kernels[FR_MAX_DEVICES];   /* render kernels launched on each device */
    float kernel_ms[FR_MAX_DEVICES];    /* their summed duration */
    uint64_t rows[FR_MAX_DEVICES];      /* rows each device rendered */
    double wall_ms;                     /* the call, entry to return */
    /* ABI 3: where each device's time went, for the first real multi-GPU run to be read against DESIGN.md 4's prediction */
    float transfer_span_ms[FR_MAX_DEVICES]; /* device time from its first transfer (DMA / ncclSend; the sink: ncclRecv) being
                                             * ready to start to its last one done; 0 for a device that moves nothing */
    double job_ms[FR_MAX_DEVICES];          /* host wall time of the device's whole job: first launch to streams drained */
    uint64_t bytes_moved[FR_MAX_DEVICES];   /* bytes the device sent to the sink (host buffer or first device's HBM) */
} fr_multi_stats;
int fr_multi_last_stats(fr_multi_stats *stats);

/* Test hook: one grouped self send/recv of `bytes` bytes through RCCL on the set's first device
 * (loads librccl, creates the communicator) — the only RCCL traffic a one-GPU box can carry. */
int fr_debug_rccl_selftest(size_t bytes);
/* Test hook: can librccl be loaded and does it export what the RCCL gather needs?  Touches no device (usable
 * without a GPU).  The environment variable FR_RCCL_LIBRARY, when set, names the library to load instead of the
 * default search — an unloadable name must yield FR_ERR_HIP and a message, never a crash. */
int fr_debug_rccl_probe(void);
/* Test hook: logical device `device_index` of the set fails before its chunk `chunk` of the NEXT multi-device
 * render (once; -1 disarms).  The render must return an error with every stream drained — no hang, no DMA
 * left in flight into the caller's buffer — and the render after it must succeed. */
int fr_debug_inject_multi_failure(int device_index, int chunk);

/* Optional, for callers that render into the SAME host buffer again and again (a GUI's frame buffer,
 * src/gui.rs:56-82): pin it once.  fr_render_rgb8 / fr_render_rgb8_multi make every large host buffer they are
 * handed DMA-able for the duration of the call (hipHostRegister, ~0.9 ms per 64 MiB) and release it before they
 * return; a buffer pinned through this call is found already registered and that cost disappears.  The library
 * does NOT cache registrations by itself: get_image returns a fresh Vec each call (src/lib.rs:266-267) and a
 * registration outliving its allocation would pin — and later DMA into — memory that belongs to someone else.
 * The caller must unpin before freeing.  Portable (valid on every device of the process). */
int fr_pin_host_buffer(void *ptr, size_t len);
int fr_unpin_host_buffer(void *ptr);

/* ---- get_image, Algo::BarnsleyFern arm — src/lib.rs:271-319, fern() :417-463 ------------------- */

/* The chaos game on the GPU.  The reference gives every rayon thread an image filled with secondary_color
 * and iterations / threads points (each point darkens the pixel it falls on: Image::subtract_pixel,
 * src/lib.rs:383-401), then "reduces" the images with combine_images — which adds a into b and returns a
 * (src/lib.rs:275-284, 305-316), so ONE thread's image comes back.  `threads` is that rayon thread count
 * (>= 1).  The reference's RNG is seeded from entropy (src/lib.rs:428): its output is a sample of a
 * distribution, and so is this one — drawn with Philox4x32-10 keyed by `seed` over `walkers` parallel
 * orbits (0 = chosen from the point count).  Deterministic for a given (seed, walkers); bit-identical to the
 * CPU restatement with the same RNG (oracle/); statistically a single sequential orbit (tests).
 * fr_render_rgb8 itself keeps rendering BarnsleyFern BLACK, as calc::get_recursive_pixel does (:211). */
int fr_render_fern_rgb8(const fr_config *cfg, uint32_t threads, uint64_t seed, uint32_t walkers, uint8_t *out,
                        size_t out_len);

/* ---- deep zoom: FR_PRECISION_DD with the low halves of the view centre ------------------------- */

/* pos_lo (NULL = (0, 0)) is the low half of the view centre: the centre is pos + pos_lo exactly, so a deep view can
 * be centred anywhere, not only on f64 grid points.  Rows [y0, y1) as r,g,b (channels 3) or r,g,b,255 (channels 4)
 * into a HOST buffer of at least channels*width*(y1-y0) bytes, or into DEVICE memory asynchronously on `hip_stream`
 * (RGBA: 4-byte aligned). */
int fr_render_rows_dd(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, int channels,
                      uint8_t *out, size_t out_len);
int fr_render_rows_dd_device(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, int channels,
                             void *d_out, size_t out_len, void *hip_stream);
/* recursive() results in DD of every pixel of rows [y0, y1) (host arrays, either may be NULL): z[4k .. 4k+3] =
 * re.hi, re.lo, im.hi, im.lo of the final position, iters[k] = escape index, k = (y-y0)*width + x. */
int fr_escape_rows_dd(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, double *z,
                      uint32_t *iters);

/* ---- deep zoom: FR_PRECISION_PT (perturbation) with the low halves of the view centre ----------------- */

/* as fr_render_rows_dd / fr_render_rows_dd_device / fr_escape_rows_dd in FR_PRECISION_PT; z holds 2 doubles per pixel
 * (z[2k] = re, z[2k+1] = im) */
int fr_render_rows_pt(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, int channels,
                      uint8_t *out, size_t out_len);
int fr_render_rows_pt_device(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, int channels,
                             void *d_out, size_t out_len, void *hip_stream);
int fr_escape_rows_pt(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, double *z,
                      uint32_t *iters);
/* FR_PRECISION_PT's reference orbit of the view, computed on the host (no device needed): which 0 = R (Mandelbrot) or V
 * (Julia), 1 = K (Julia only).  *len receives the number of entries; min(*len, cap) of them are written to out as
 * re, im pairs (2 doubles per entry). */
int fr_debug_reference_orbit(const fr_config *cfg, const fr_imaginary *pos_lo, int which, double *out, size_t cap,
                             uint32_t *len);

/* ---- supersampled rendering: render s times as large, box-filter on the device ------------------------ */

/* The reference's own remedy for "the aliasing of the borders" (--unsmooth's help text) is to render large and scale
 * down (its README screenshot is a 3000 x 3000 render shown at 1000 x 1000).  Here that happens on the device, so that
 * only the small image crosses PCIe and the large one never exists whole.  DEFINITION, for supersample = s,
 * 1 <= s <= FR_SS_MAX:
 *   cfg_s = cfg with width * s and height * s, every other field unchanged;
 *   H     = the image of cfg_s at the requested precision (with pos_lo for DD and PT): the bytes
 *           fr_render_rows_rgb8 / fr_render_rows_dd / fr_render_rows_pt produce for cfg_s;
 *   out(X, Y, c) = (sum over j < s, i < s of H(s*X + i, s*Y + j, c) + floor(s*s / 2)) / (s*s)
 *           in integer arithmetic, truncating (the sums fit in 16 bits); with 4 channels alpha is 255.
 * s = 1 is the plain render, byte for byte.  Algo::BarnsleyFern stays black.
 * This is literally "render s times as large and box-filter": the s*s samples of pixel (X, Y) cover [X, X+1) x [Y, Y+1)
 * from its top-left corner, so the image sits (s-1)/(2s) of a pixel away (right and down) from the s = 1 render, whose one
 * sample is that corner.
 * Domain (else FR_ERR_INVALID_ARGUMENT, before any device work): s in 1 .. FR_SS_MAX; s * width and s * height fit in
 * 32 bits; the precision's own domain on cfg_s; pos_lo non-NULL only for DD and PT; channels 3 or 4.  One device. */
#define FR_SS_MAX 8

/* Workspace of fr_render_rows_ss_device for rows [y0, y1): rows [s*y0, s*y1) of cfg_s are rendered in bands of B source
 * rows (packed r,g,b, 3 * s * width bytes a row) into the workspace, each band filtered into its place in the output.
 * *min_bytes = one band of 8 * s source rows (or all the rows if there are fewer); *best_bytes = the whole range, at most
 * 1 GiB (never under *min_bytes).  Any length from *min_bytes up is accepted and used: Bmax = the multiple of 8 * s rows
 * that fit (or all the rows), nb = ceil(rows / Bmax) bands, B = ceil(rows / nb) rounded up to 8 * s — whole tile rows and
 * whole output rows per band, no sliver at the end.  s = 1: both 0.  Either pointer may be NULL.  No device needed. */
int fr_ss_workspace_bytes(const fr_config *cfg, uint32_t supersample, uint32_t y0, uint32_t y1, size_t *min_bytes,
                          size_t *best_bytes);
/* Rows [y0, y1) of the supersampled image as r,g,b (channels 3) or r,g,b,255 (channels 4; d_out 4-byte aligned) into
 * DEVICE memory, asynchronously on `hip_stream`.  The caller lends the workspace d_work (device memory, work_len bytes,
 * any alignment; NULL / 0 for s = 1) until the work queued on the stream has finished; the library allocates nothing and
 * takes no lock beyond its slot rings: re-entrant, each thread with a workspace and a stream of its own.  A work_len
 * under *min_bytes gives FR_ERR_BUFFER_TOO_SMALL.  F64 and F32 choose ONE kernel for the whole source range (as the
 * bands of the host path do); PT computes the view's orbit once.  With profiling on, fr_last_kernel_ms returns the span
 * of the whole call on the stream, first band's kernel to last filter, and fr_last_kernel_name the render kernel. */
int fr_render_rows_ss_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample,
                             uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work,
                             size_t work_len, void *hip_stream, const fr_render_opts *opts);
/* The same into a HOST buffer of at least channels*width*(y1-y0) bytes.  The workspace (at most 256 MiB) and the result
 * live in the context's scratch memory; the result leaves the device in one copy: only the small image crosses PCIe.
 * y0 == y1 is legal (no-op) without a device. */
int fr_render_rows_ss(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample, uint32_t y0,
                      uint32_t y1, int channels, uint8_t *out, size_t out_len, const fr_render_opts *opts);
/* The filter alone — e.g. over a large render the caller already holds: src = packed r,g,b rows of supersample * width
 * pixels, supersample * rows of them; out = `rows` packed rows of `width` pixels, channels 3 or 4 (out_len >=
 * channels*width*rows).  Host arrays, or device arrays (any alignment; RGBA output 4-byte aligned) + stream for the
 * _device form. */
int fr_box_filter_rgb8(const uint8_t *src, uint32_t width, uint32_t rows, uint32_t supersample, int channels, uint8_t *out,
                       size_t out_len);
int fr_box_filter_rgb8_device(const void *d_src, uint32_t width, uint32_t rows, uint32_t supersample, int channels,
                              void *d_out, size_t out_len, void *hip_stream);

/* ---- get_recursive_pixel — calc/src/lib.rs:199-235 ---------------------------------------- */

int fr_pixel(const fr_config *cfg, uint32_t x, uint32_t y, fr_rgb *out);
int fr_pixel_p(const fr_config *cfg, int precision, uint32_t x, uint32_t y, fr_rgb *out);

/* ---- recursive — calc/src/lib.rs:245-257 --------------------------------------------------- */

/* One orbit: returns the final position and the escape index (== iterations on exhaustion). */
int fr_recursive(uint32_t iterations, fr_imaginary start, fr_imaginary c, double limit,
                 fr_imaginary *out_pos, uint32_t *out_iters);

/* n independent orbits (host arrays): start[k], c[k] -> out_pos[k], out_iters[k]. */
int fr_recursive_batch(uint32_t iterations, const fr_imaginary *start, const fr_imaginary *c, size_t n,
                       double limit, int precision, fr_imaginary *out_pos, uint32_t *out_iters);

/* recursive() results of every pixel of rows [y0, y1) (host arrays, either may be NULL):
 * z_re_im[2k], z_re_im[2k+1] = final position, iters[k] = escape index, k = (y-y0)*width + x. */
int fr_escape_rows(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, double *z_re_im,
                   uint32_t *iters);

/* The colour map alone (calc/src/lib.rs:214-234 + color_multiply) over n stored recursive() results
 * — e.g. the arrays fr_escape_rows returned — into packed r,g,b.  This is what the GUI's exposure,
 * smooth/inside and colour controls need (src/gui.rs:183-203 change only inputs of the colour map):
 * re-colouring without re-iterating.  Uses cfg's iterations, stable_limit, exposure, inside, smooth
 * and colours; host arrays, or device arrays + stream for the _device form. */
int fr_colour_rgb8(const fr_config *cfg, const double *z_re_im, const uint32_t *iters, size_t n, uint8_t *out,
                   size_t out_len);
int fr_colour_rgb8_device(const fr_config *cfg, const void *d_z_re_im, const void *d_iters, size_t n, void *d_out,
                          size_t out_len, void *hip_stream);

/* ---- a view kept on the device: raw results, a higher cap, colours ------------------------------------ */

/* A GUI keeps (z, iters) of the current view in DEVICE memory — 20 bytes per pixel, 36 for DD with its low parts — and
 * answers an iterations change with fr_escape_extend_device and every control that only feeds the colour map (exposure,
 * colours, smooth, inside) with fr_colour_rows_device; only pan, zoom and limit need new orbits.  The device forms are
 * asynchronous on `hip_stream`, allocate nothing, take no lock beyond what the render they wrap takes (PT: the context's
 * orbit cache), are re-entrant, and the caller owns every buffer. */

/* recursive() results of rows [y0, y1) into DEVICE arrays: what fr_escape_rows / _dd / _pt copy to the host.
 * z_width 2: re, im (DD: the hi parts); z_width 4: re.hi, re.lo, im.hi, im.lo (FR_PRECISION_DD only).
 * d_z: z_width doubles per pixel, 8-byte aligned; d_iters: uint32 per pixel; either may be NULL; k = (y-y0)*width + x.
 * pos_lo non-NULL only for DD and PT.  opts: NULL = defaults (selects what fr_escape_rows' launch takes: tile, loop_mode). */
int fr_escape_rows_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1,
                          int z_width, void *d_z, void *d_iters, void *hip_stream, const fr_render_opts *opts);

/* Raise the iteration cap of stored results IN PLACE.  DEFINITION, with N = from_iterations, M = cfg->iterations and
 * cfg_N = cfg with iterations = N:
 *   Precondition: the arrays hold what fr_escape_rows_device(cfg_N, precision, pos_lo, y0, y1, z_width, ...) writes.
 *   Result: after the call they hold what the same call writes for cfg, bit for bit, z and iters alike.
 *   A pixel with iters[k] != N is finished: only its iters[k] is read, nothing of it is written, its z is never loaded.
 *   Values of iters[k] above N are foreign data and are left alone like finished pixels.
 * The library CANNOT check the precondition: arrays that come from another view, precision or cap are continued as if
 * they were this one's, and the result is then whatever that orbit gives.  Nor is the call idempotent: in arrays that
 * already hold cap M, iters[k] == N means "escaped at step N", and a second call N -> M would continue those orbits.
 * Why the bytes are the render's: recursive() (calc/src/lib.rs:245-257) returns `previous` after exactly N steps when the
 * cap is reached — the loop's whole state — and c is a function of the pixel, recomputed by the render's own coordinate
 * code; continuing for M - N steps is the loop at cap M.
 * Domain (else FR_ERR_INVALID_ARGUMENT, before any device work): M >= N — M == N is a legal no-op that needs no device; a
 * lower cap cannot be derived from stored results.  FR_PRECISION_F64 and FR_PRECISION_F32 take z_width 2 (for F32 the
 * stored doubles are widened f32 values, and narrowing them back is exact); FR_PRECISION_DD takes z_width 4 only — the low
 * parts are state — with DD's domain on cfg and pos_lo.  FR_PRECISION_PT is refused: its per-pixel state is (X, m, dz), not
 * z, and the step at which a pixel meets "m == last of X" depends on the cap (the orbit's length does), so a stored z does
 * not determine the continuation (fr_escape_rows_pt_state_device / fr_escape_extend_pt_device below keep and continue
 * that state).  Both d_z and d_iters are required (y0 == y1 needs neither).  pos_lo non-NULL only for
 * DD.  opts: NULL = defaults; loop_mode 5 = no speculative blocks (same bytes).
 * With profiling on, fr_last_kernel_name reports escape_extend_kernel<double> / <float> / escape_extend_dd_kernel. */
int fr_escape_extend_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1,
                            uint32_t from_iterations, int z_width, void *d_z, void *d_iters, void *hip_stream,
                            const fr_render_opts *opts);
/* the same over HOST arrays (upload, extend, download, synchronise; scratch from the context as fr_colour_rgb8 does) */
int fr_escape_extend(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1,
                     uint32_t from_iterations, int z_width, double *z, uint32_t *iters);

/* The colour map over stored results in DEVICE memory: channels 3 (r,g,b) or 4 (r,g,b,255; d_out 4-byte aligned),
 * z_width 2 or 4 (colour on the hi parts, as the DD definition says).  out_len >= channels * n. */
int fr_colour_rows_device(const fr_config *cfg, const void *d_z, int z_width, const void *d_iters, size_t n, int channels,
                          void *d_out, size_t out_len, void *hip_stream);

/* ---- statistics of a kept view: where its pixels escape, and the exposure that shows it ---------------- */

/* The colour map is primary * (iters [+ 1 - nu]) / iterations * exposure (calc/src/lib.rs:228) with `exposure` a constant of
 * the Config that suits the default view at 50 iterations; a deep view needs a cap in the thousands while its pixels escape
 * in a narrow band far below it, and comes out nearly flat.  The reference leaves that to a person at the GUI's exposure
 * control (src/gui.rs:183-203).  These calls reduce a kept view's (z, iters) ON THE DEVICE to a small record — 8 KB cross
 * PCIe, not 20 bytes per pixel — from which two host helpers take a percentile of the escape indices and the exposure that
 * maps it to the full primary colour; the image is then fr_colour_rows_device's at that exposure, the reference's own colour
 * map byte for byte.  DEFINITION, for pixel k of n:
 *   re, im = the f64 position the colour map reads: z[2k], z[2k+1] for z_width 2; the hi parts z[4k], z[4k+2] for z_width 4;
 *   dist   = re*re + im*im: two f64 multiplications and one addition, nothing fused (what the colour map forms);
 *   it = iters[k], N = cfg->iterations.
 *   Classes — the colour map's own branches (calc/src/lib.rs:216):
 *     S (stable)  !(dist > cfg->stable_limit); a NaN dist lands here, as it does in the colour map;
 *     C (capped)  dist > stable_limit and it >= N: exhaustion; foreign values above N count here too;
 *     E (escaped) dist > stable_limit and it < N.
 *   min_iters, max_iters, sum_iters are taken over E; shift is the smallest s >= 0 with (max_iters - min_iters) >> s <
 *   FR_STATS_BINS; hist[b] is the number of pixels of E with (it - min_iters) >> shift == b.
 * Every field is an integer function of the input: the result is bit-exact and independent of launch shape and atomic
 * order.  Only cfg->iterations and cfg->stable_limit are read; algo, precision and the road that produced the arrays do not
 * matter.  One call covers one array: records of row pieces are not merged, and multi-device / block-cyclic views are out
 * of scope. */
/* The record is a struct TAG, not a typedef: the call that fills it bears the same name, and in C a typedef and a function
 * cannot share one.  Write `struct fr_view_stats` (in C++ too, where the function hides the bare name). */
#define FR_STATS_BINS 1024
struct fr_view_stats { /* sizeof == 8248 */
    uint64_t n;         /* pixels examined */
    uint64_t stable;    /* class S */
    uint64_t capped;    /* class C */
    uint64_t escaped;   /* class E;  n == stable + capped + escaped */
    uint64_t sum_iters; /* sum of iters over class E, modulo 2^64 */
    uint32_t min_iters; /* over class E; 0 when escaped == 0 */
    uint32_t max_iters; /* over class E; 0 when escaped == 0 */
    uint32_t shift;     /* a bin is 2^shift escape indices wide; 0 when escaped == 0 */
    uint32_t reserved;  /* 0 */
    uint64_t hist[FR_STATS_BINS];
};

/* Device arrays, asynchronous on hip_stream; d_stats: device memory, sizeof(struct fr_view_stats) bytes, 8-byte aligned.  The
 * call overwrites *d_stats whatever it held (no precondition), allocates nothing, takes no lock, is re-entrant.  n == 0 is
 * legal: an all-zero record with n = 0 (still queued on the stream: d_stats is device memory).
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): non-NULL pointers (the arrays may be NULL
 * only when n == 0); z_width 2 or 4; d_z 8-byte, d_iters 4-byte, d_stats 8-byte aligned; n <= 2^40; stable_limit not NaN. */
int fr_view_stats_device(const fr_config *cfg, const void *d_z, int z_width, const void *d_iters, size_t n, void *d_stats,
                         void *hip_stream);
/* the same over HOST arrays into a host record (context scratch: upload, launch, one small download, synchronise — as
 * fr_colour_rgb8 does); n == 0 needs no device */
int fr_view_stats(const fr_config *cfg, const double *z, int z_width, const uint32_t *iters, size_t n,
                  struct fr_view_stats *out);
/* Host only, no device.  The escape index at quantile p of class E: escaped == 0 gives 0; otherwise
 * k = ceil(p * (double)escaped) — one f64 multiplication — clamped to [1, escaped], b = the smallest bin whose cumulative
 * count reaches k, and the result is min(max_iters, min_iters + ((b + 1) << shift) - 1) computed in 64 bits: the bin's last
 * index, exact when shift == 0.
 * Domain: non-NULL pointers; p finite in [0, 1]; a self-consistent record (shift < 32, min_iters <= max_iters, and a
 * histogram that reaches k). */
int fr_stats_percentile(const struct fr_view_stats *s, double p, uint32_t *iters_out);
/* Host only, no device.  escaped == 0 gives cfg->exposure; otherwise q = max(fr_stats_percentile(s, p), 1) and
 * exposure = (double)cfg->iterations / (double)q, one f64 division: an escaped pixel at the p-quantile then has
 * iters / iterations * exposure at (or one rounding under) 1 and gets the full primary colour.  With `smooth` the 1 - nu
 * term shifts every pixel by the same 2 to 3 indices; that is accepted, the definition is on the escape index.
 * Domain: fr_stats_percentile's, and cfg not NULL. */
int fr_auto_exposure(const fr_config *cfg, const struct fr_view_stats *s, double p, double *exposure_out);

/* ---- resumable perturbation: a deep view's cap raised in place ----------------------------------------- */

/* A GUI keeps a PT view as (z, iters, dz, m) in DEVICE memory — 40 bytes per pixel — and answers an iterations change with
 * fr_escape_extend_pt_device; fr_colour_rows_device over (z, iters) with z_width 2 colours it.  The definition of the state
 * and why continuing it is the render at the higher cap: fr_precision above, "RESUMABLE PT".  The library keeps the view's
 * reference orbits per context and CONTINUES them for a higher cap of the same view: orbits that are all ended by escape
 * are served as they are; otherwise only the missing entries are computed on the host, from the stored dd tail. */

/* Rows [y0, y1) in FR_PRECISION_PT with their resumable state into DEVICE arrays, asynchronously on `hip_stream`:
 * d_z, d_dz 2 doubles per pixel (re, im), 8-byte aligned; d_iters, d_m one uint32 per pixel, 4-byte aligned; all four
 * required (y0 == y1 needs none and no device); k = (y-y0)*width + x.  d_z and d_iters receive what fr_escape_rows_pt gives,
 * bit for bit.  Domain: FR_PRECISION_PT's on cfg and pos_lo.  An algorithm without orbits (BarnsleyFern) writes zeros.
 * With profiling on, fr_last_kernel_name reports escape_pt_state_kernel. */
int fr_escape_rows_pt_state_device(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, void *d_z,
                                   void *d_iters, void *d_dz, void *d_m, void *hip_stream);
/* Raise the cap of a stored state IN PLACE, N = from_iterations -> M = cfg->iterations, cfg_N = cfg with iterations = N:
 *   Precondition: the arrays hold what fr_escape_rows_pt_state_device(cfg_N, pos_lo, y0, y1, ...) writes.
 *   Result: after the call they hold what the same call writes for cfg, bit for bit in all four arrays.
 *   A pixel with iters[k] != N is finished: only that word is read; its z, dz and m are neither loaded nor written.  Values
 *   of iters[k] above N are foreign data and are left alone like finished pixels.
 * The library CANNOT check the precondition: arrays from another view or cap are continued as if they were this one's (an
 * index m beyond the orbit is brought inside it, nothing more).  Nor is the call idempotent: in arrays that already hold
 * cap M, iters[k] == N means "escaped at step N", and a second call N -> M would continue those pixels.
 * Domain (else FR_ERR_INVALID_ARGUMENT, before any device work): M >= N — M == N is a legal no-op that needs no device;
 * FR_PRECISION_PT's domain on cfg (with iterations <= FR_PT_MAX_ITERATIONS) and pos_lo; all four arrays, aligned as above
 * (y0 == y1 needs none).  An algorithm without orbits: nothing is done.
 * With profiling on, fr_last_kernel_name reports escape_extend_pt_kernel. */
int fr_escape_extend_pt_device(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1,
                               uint32_t from_iterations, void *d_z, void *d_iters, void *d_dz, void *d_m, void *hip_stream);
/* the same over HOST arrays (context scratch; upload, launch, download, synchronise, as fr_escape_extend does) */
int fr_escape_rows_pt_state(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, double *z,
                            uint32_t *iters, double *dz, uint32_t *m);
int fr_escape_extend_pt(const fr_config *cfg, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, uint32_t from_iterations,
                        double *z, uint32_t *iters, double *dz, uint32_t *m);
/* Test hook: out[0] = the iterations the context's cached PT orbit is for, out[1] / out[2] = entries of X / K (K: Julia
 * only), out[3] = entries the last request for it computed on the host (0 = served as it was).  Zeros without a cached
 * orbit.  Touches no device. */
int fr_debug_pt_orbit_cache(uint32_t out[4]);

/* ---- WIDE PT: perturbation with a fixed-point view centre of up to 1016 bits ----------------------------------- */

/* The view centre of WIDE PT (fr_precision above, "WIDE PT"): re and im point to n_words little-endian uint64_t words each,
 * two's complement, value I / 2^(64 n_words - 8).  The caller owns the words; the library copies what it keeps. */
typedef struct fr_wide_centre { uint32_t n_words; const uint64_t *re; const uint64_t *im; } fr_wide_centre;

/* Host-only helpers on one component (w: n words, 2 <= n <= FR_WIDE_MAX_WORDS); none needs a device.  Each refuses, with
 * FR_ERR_INVALID_ARGUMENT and w unchanged, a result outside |v| <= 2, a non-finite input and an n out of range.
 *   fr_wide_from_double   w = floor(v 2^F): exact whenever v is representable.
 *   fr_wide_add_double    I += floor(delta 2^F): a pan step, or a clicked pixel's off, added to the centre.
 *   fr_wide_to_double     *hi = the f64 nearest to the value (ties to even), *lo (may be NULL) = the f64 nearest to the rest
 *                         (at most half an ulp of *hi): a (pos, pos_lo) pair, which hands the view over to PT or DD at
 *                         shallow scales.
 *   fr_wide_from_decimal  w = floor of the decimal's exact value: [+-]digits[.digits][e[+-]digits] (at least one digit, at
 *                         most four in the exponent, nothing else — no blanks); a malformed string is refused. */
int fr_wide_from_double(double v, uint64_t *w, uint32_t n);
int fr_wide_add_double(uint64_t *w, uint32_t n, double delta);
int fr_wide_to_double(const uint64_t *w, uint32_t n, double *hi, double *lo);
int fr_wide_from_decimal(const char *text, uint64_t *w, uint32_t n);

/* Each call is the exact counterpart of the PT call it is named after, with `centre` where that one takes pos_lo (and
 * cfg->pos): fr_render_rows_pt / _device, fr_escape_rows_pt, fr_escape_rows_pt_state(_device), fr_escape_extend_pt(_device)
 * — the same buffers, alignment, asynchrony, precondition / result contract of the extension (a finished pixel has only its
 * iters word read; M == N is a no-op that needs no device; y0 == y1 needs none either).  Domain: WIDE PT's.  The context's
 * single orbit slot serves both roads: a wide view is told from a dd view and from a wide view with other words or another
 * n, and raising the cap of the same wide view computes only the missing entries, from the orbit's last entry kept as
 * integers (nothing when every orbit is ended by escape).  fr_debug_pt_orbit_cache reports a wide orbit the same way. */
int fr_render_rows_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, int channels,
                           uint8_t *out, size_t out_len);
int fr_render_rows_pt_wide_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, int channels,
                                  void *d_out, size_t out_len, void *hip_stream);
int fr_escape_rows_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z,
                           uint32_t *iters);
int fr_escape_rows_pt_wide_state_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, void *d_z,
                                        void *d_iters, void *d_dz, void *d_m, void *hip_stream);
int fr_escape_extend_pt_wide_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                                    uint32_t from_iterations, void *d_z, void *d_iters, void *d_dz, void *d_m, void *hip_stream);
int fr_escape_rows_pt_wide_state(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z,
                                 uint32_t *iters, double *dz, uint32_t *m);
int fr_escape_extend_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, uint32_t from_iterations,
                             double *z, uint32_t *iters, double *dz, uint32_t *m);
/* WIDE PT's reference orbit of the view on the host (no device needed), as fr_debug_reference_orbit: which 0 = R or V,
 * 1 = K (Julia only); *len = the number of entries, min(*len, cap) of them written to out as re, im pairs. */
int fr_debug_reference_orbit_wide(const fr_config *cfg, const fr_wide_centre *centre, int which, double *out, size_t cap,
                                  uint32_t *len);

/* ---- BLA-PT: perturbation that skips iterations in bulk -------------------------------------------------------- */

/* The BLA-PT calls (fr_precision above, "BLA-PT").  One road for both centres: `centre` non-NULL selects WIDE PT's orbits
 * (pos_lo must then be NULL and cfg->pos is not read), otherwise the centre is PT's (cfg->pos, pos_lo), pos_lo NULL = (0, 0).
 * bits: 0 = FR_BLA_DEFAULT_BITS, else 24 .. 53.  y0 == y1 and argument errors need no device.  The library builds the view's
 * table on the host from the orbit PT's cache holds (computing it on a miss), uploads it once and keeps it per context beside
 * the orbit, keyed by that orbit, D and bits: the same view with other rows or colours is served, anything else rebuilds.  PT
 * and BLA-PT calls may alternate on one context.
 * fr_render_rows_pt_bla(_device): the buffers, alignment and asynchrony of fr_render_rows_pt(_device).
 * fr_escape_rows_pt_bla(_device): z is 2 doubles per pixel (re, im), as fr_escape_rows_pt / fr_escape_rows_device give it;
 * fr_colour_rgb8 / fr_colour_rows_device over them reproduces the render.  With profiling on, fr_last_kernel_name reports
 * escape_bla_kernel. */
int fr_render_rows_pt_bla(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                          uint32_t y1, int channels, uint8_t *out, size_t out_len);
int fr_render_rows_pt_bla_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits,
                                 uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *hip_stream);
int fr_escape_rows_pt_bla(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                          uint32_t y1, double *z, uint32_t *iters);
int fr_escape_rows_pt_bla_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits,
                                 uint32_t y0, uint32_t y1, void *d_z, void *d_iters, void *hip_stream);
/* Host only, no device: level `level` of the table of orbit `which` (0: R or V, 1: K, Julia only).  *len = n_level, or 0 past
 * the top; min(*len, cap) entries are written to out as 5 doubles: A.re, A.im, B.re, B.im, r2. */
int fr_debug_bla_table(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, int which,
                       uint32_t level, double *out, size_t cap, uint32_t *len);
/* On the device: over the pixels of rows [y0, y1), *passes = the passes through the BLA loop (each a plain step or one skip)
 * and *steps = the nominal iterations (escape index + 1, or the cap): their ratio is what the skips save. */
int fr_debug_bla_count(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                       uint32_t y1, uint64_t *passes, uint64_t *steps);
/* Test hook: out[0] = bits of the context's cached table, out[1] = levels of X's table (level 0 included), out[2] = entries
 * of all levels of X's and K's tables, out[3] = 1 if the last request built the table, 0 if it was served.  Zeros without a
 * cached table.  Touches no device. */
int fr_debug_bla_cache(uint32_t out[4]);

/* ---- SCALED PT: WIDE PT and BLA-PT down to a scale of 2^951 -------------------------------------------------------- */

/* The SCALED PT calls (fr_precision above, "SCALED PT").  `centre` is required; cfg->pos is not read.  bits: -1 = no table
 * (the plain scaled loop, WIDE PT's counterpart), 0 = FR_BLA_DEFAULT_BITS, else 24 .. 53 (BLA-PT's counterpart).  y0 == y1 and
 * argument errors need no device.  The orbit is the one the fr_*_pt_wide calls cache (either road serves the other); the
 * table is built, uploaded and kept per context as BLA-PT's is, in the same slot, keyed by the orbit, Dw, S, bits and its kind
 * (S = 2^e on its own: a scale 2^k times another's has the same orbit and Dw, and every radius 2^k times as large).
 * fr_render_rows_pt_scaled(_device): the buffers, channels, alignment and asynchrony of fr_render_rows_pt_wide(_device).
 * fr_escape_rows_pt_scaled(_device): as fr_escape_rows_pt_bla(_device); fr_colour_rgb8 / fr_colour_rows_device over the
 * results reproduces the render.  With profiling on, fr_last_kernel_name reports escape_pt_scaled_kernel (bits = -1) or
 * escape_bla_scaled_kernel. */
int fr_render_rows_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, int channels,
                             uint8_t *out, size_t out_len);
int fr_render_rows_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1,
                                    int channels, void *d_out, size_t out_len, void *hip_stream);
int fr_escape_rows_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, double *z,
                             uint32_t *iters);
int fr_escape_rows_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1,
                                    void *d_z, void *d_iters, void *hip_stream);
/* Host only, no device: as fr_debug_bla_table for the scaled table (bits 0 or 24 .. 53); 5 doubles per entry: A.re, A.im,
 * B.re, B.im and the stored R. */
int fr_debug_bla_table_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, int which, uint32_t level, double *out,
                              size_t cap, uint32_t *len);
/* On the device, as fr_debug_bla_count: *passes = the passes through the scaled loop (bits = -1: one per step), *steps = the
 * nominal iterations. */
int fr_debug_pt_scaled_count(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1,
                             uint64_t *passes, uint64_t *steps);

/* RESUMABLE SCALED PT (fr_precision above): a GUI keeps a view past 2^440 as (z, iters, w, m) in DEVICE memory — 40 bytes per
 * pixel — and answers an iterations change with fr_escape_extend_pt_scaled_device; fr_colour_rows_device over (z, iters) with
 * z_width 2 colours it.  The calls are the plain scaled loop's and take no bits.  Each is the exact counterpart of the
 * fr_*_pt_wide call it is named after, with d_w / w where that one has d_dz / dz: the same buffers, alignment and asynchrony
 * on `hip_stream`, nothing allocated, and the same precondition / result contract of the extension.
 *   fr_escape_rows_pt_scaled_state(_device): rows [y0, y1) with their state; d_z, d_w 2 doubles per pixel (re, im), 8-byte
 *   aligned; d_iters, d_m one uint32 per pixel, 4-byte aligned; all four required (y0 == y1 needs none and no device);
 *   k = (y-y0)*width + x.  d_z and d_iters receive what fr_escape_rows_pt_scaled gives with bits = -1, bit for bit.  An
 *   algorithm without orbits (BarnsleyFern) writes zeros.  fr_last_kernel_name reports escape_pt_scaled_state_kernel.
 *   fr_escape_extend_pt_scaled(_device): raise the cap of a stored state IN PLACE, N = from_iterations -> M = cfg->iterations,
 *   cfg_N = cfg with iterations = N.
 *     Precondition: the arrays hold what fr_escape_rows_pt_scaled_state_device(cfg_N, centre, y0, y1, ...) writes.
 *     Result: after the call they hold what the same call writes for cfg, bit for bit in all four arrays.
 *     A pixel with iters[k] != N is finished: only that word is read; its z, w and m are neither loaded nor written.  Values
 *     of iters[k] above N are foreign data and are left alone like finished pixels.
 *   The library CANNOT check the precondition: arrays from another view or cap — or a state of the fr_*_pt_wide_state calls,
 *   which holds dz, not w — are continued as if they were this view's (an index m beyond the orbit is brought inside it,
 *   nothing more).  Nor is the call idempotent: in arrays that already hold cap M, iters[k] == N means "escaped at step N",
 *   and a second call N -> M would continue those pixels.  M == N is a legal no-op that needs no device; an algorithm without
 *   orbits: nothing is done.  fr_last_kernel_name reports escape_extend_pt_scaled_kernel.
 * The orbit is the shared slot's: raising the cap of a scaled view computes only the missing entries, from the orbit's last
 * entry kept as integers, and nothing when every orbit is ended by escape (fr_debug_pt_orbit_cache shows it).  The host
 * forms go through the context's scratch: upload (extension), launch, download, synchronise. */
int fr_escape_rows_pt_scaled_state_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, void *d_z,
                                          void *d_iters, void *d_w, void *d_m, void *hip_stream);
int fr_escape_extend_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                                      uint32_t from_iterations, void *d_z, void *d_iters, void *d_w, void *d_m, void *hip_stream);
int fr_escape_rows_pt_scaled_state(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z,
                                   uint32_t *iters, double *w, uint32_t *m);
int fr_escape_extend_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, uint32_t from_iterations,
                               double *z, uint32_t *iters, double *w, uint32_t *m);

/* ---- supersampled rendering on the deep roads: WIDE PT, BLA-PT, SCALED PT --------------------------------------- */

/* fr_render_rows_ss(_device) above take (precision, pos_lo) only; these two take the deep roads' own arguments.  DEFINITION,
 * for supersample = s, 1 <= s <= FR_SS_MAX — the "supersampled rendering" block's, word for word, with H per road:
 *   cfg_s = cfg with width * s and height * s, every other field unchanged;
 *   H     = the image of cfg_s on the road:
 *             FR_PT_ROAD_PLAIN, centre == NULL   the bytes of fr_render_rows_pt(cfg_s, pos_lo, ...) — this case equals
 *                                                fr_render_rows_ss with FR_PRECISION_PT, byte for byte; pos_lo optional,
 *                                                bits must be 0;
 *             FR_PT_ROAD_PLAIN, centre != NULL   fr_render_rows_pt_wide(cfg_s, centre, ...); pos_lo must be NULL, bits 0;
 *             FR_PT_ROAD_BLA                     fr_render_rows_pt_bla(cfg_s, pos_lo, centre, bits, ...); pos_lo / centre as
 *                                                BLA-PT takes them, bits 0 or 24 .. 53;
 *             FR_PT_ROAD_SCALED                  fr_render_rows_pt_scaled(cfg_s, centre, bits, ...); centre required, pos_lo
 *                                                NULL, bits -1, 0 or 24 .. 53;
 *   out(X, Y, c) = (sum over j < s, i < s of H(s*X + i, s*Y + j, c) + floor(s*s / 2)) / (s*s)
 *           in integer arithmetic, truncating (the sums fit in 16 bits); with 4 channels alpha is 255.
 * s = 1 is the road's plain render, byte for byte.  Algo::BarnsleyFern stays black.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message, before any device work): s in 1 .. FR_SS_MAX; s * width and s * height
 * fit in 32 bits; road in 0 .. 2; channels 3 or 4; the road's own domain ON cfg_s, checked by the code its plain calls run —
 * D and Dw are taken over the whole image of cfg_s, as the definition of H says, and the F >= e + 64 rule reads cfg's scale,
 * which cfg_s shares.
 * Buffers: exactly fr_render_rows_ss(_device)'s — fr_ss_workspace_bytes serves these calls too (it depends on cfg, s and the
 * rows only); work_len under *min_bytes or a short out_len give FR_ERR_BUFFER_TOO_SMALL; RGBA output is 4-byte aligned;
 * d_work NULL / 0 for s = 1; y0 == y1 is a no-op without a device.
 * The device form is asynchronous on `hip_stream`, allocates nothing and takes no lock beyond what the road's plain device
 * call takes (the orbit / table cache): the orbit — and for BLA and SCALED-with-table the table — is computed and uploaded by
 * the first band and served to the others (the caches are keyed by the view, not by the rows).  The host form uses the
 * context's scratch (workspace at most 256 MiB) and one device-to-host copy of the small image.  With profiling on,
 * fr_last_kernel_name reports the road's kernel and fr_last_kernel_ms the span from the first band's kernel to the last
 * filter. */
typedef enum fr_pt_road { FR_PT_ROAD_PLAIN = 0, FR_PT_ROAD_BLA = 1, FR_PT_ROAD_SCALED = 2 } fr_pt_road;
int fr_render_rows_ss_pt_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                                uint32_t supersample, uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len,
                                void *d_work, size_t work_len, void *hip_stream);
int fr_render_rows_ss_pt(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                         uint32_t supersample, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len);

/* A KEPT anti-aliased view is a kept view of cfg_s: (z, iters) of the s times larger image in DEVICE memory, written by any
 * fr_escape_rows*_device call for cfg_s on any road and kept current by the extend calls.  This colours and filters it in ONE
 * kernel, with no RGB workspace (the two-call composition needs 3 * s * s bytes per output pixel).  DEFINITION: the arrays
 * hold s * rows rows of s * width samples, k = Y * (s * width) + X; then
 *   out = fr_box_filter_rgb8(fr_colour_rows(cfg, z, z_width, iters, n = s*s * width * rows), width, rows, s, channels),
 * byte for byte.  cfg contributes only what the colour map reads (iterations, stable_limit, exposure, inside, smooth, the
 * colours, algo); an algorithm without orbits gives black; s = 1 is fr_colour_rows_device.
 * Domain: z_width 2 or 4 (colour on the hi parts); channels 3 or 4 (RGBA output 4-byte aligned); s in 1 .. FR_SS_MAX with
 * s * width and s * rows in 32 bits; d_z 8-byte aligned, d_iters 4-byte aligned; out_len >= channels * width * rows
 * (FR_ERR_BUFFER_TOO_SMALL); an empty output (width or rows 0) is a no-op without a device.  The device form is asynchronous
 * on `hip_stream`, allocates nothing and takes no lock.  fr_colour_ss_rgb8: the same over HOST arrays (upload to context
 * scratch, launch, download, synchronise, as fr_colour_rgb8 does). */
int fr_colour_rows_ss_device(const fr_config *cfg, const void *d_z, int z_width, const void *d_iters, uint32_t width, uint32_t rows,
                             uint32_t supersample, int channels, void *d_out, size_t out_len, void *hip_stream);
int fr_colour_ss_rgb8(const fr_config *cfg, const double *z, int z_width, const uint32_t *iters, uint32_t width, uint32_t rows,
                      uint32_t supersample, int channels, uint8_t *out, size_t out_len);

/* ---- distance estimation: the orbit's derivative, the distance in pixels, distance-shaded colour ----------- */

/* DE (defined at fr_precision above).  A kept view gains one array: der, 2 doubles per pixel beside (z, iters) — 36 bytes per
 * pixel in all.  Thickness, like exposure, is then a recolour: fr_colour_de_rows_device over the kept arrays, no orbit.
 * The _device forms are asynchronous on hip_stream, allocate nothing and take no lock beyond what the road's render takes
 * (PT: the context's orbit cache, which they share with the PT calls: no second orbit is computed).
 *
 * Rows [y0, y1) of the view with their derivatives: z and der 2 doubles per pixel (8-byte aligned), iters uint32 (4-byte
 * aligned), k = (y - y0) * width + x.  All three arrays are required; y0 == y1 is a no-op that needs no device.  precision:
 * FR_PRECISION_F64 (pos_lo must be NULL) or FR_PRECISION_PT (pos_lo NULL = (0, 0)).  With profiling on, fr_last_kernel_name
 * reports escape_de_kernel / escape_pt_de_kernel. */
int fr_escape_rows_de_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, void *d_z,
                             void *d_iters, void *d_der, void *hip_stream);
int fr_escape_rows_de(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t y0, uint32_t y1, double *z,
                      uint32_t *iters, double *der);
/* the same on PT with a wide centre (WIDE PT's domain; centre required) */
int fr_escape_rows_de_pt_wide_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, void *d_z,
                                     void *d_iters, void *d_der, void *hip_stream);
int fr_escape_rows_de_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z,
                              uint32_t *iters, double *der);
/* DE ON BLA-PT (defined at fr_precision above): rows [y0, y1) with their derivatives on the BLA-PT road; the centre convention
 * is the fr_*_pt_bla calls' (a dd centre (cfg->pos, pos_lo), pos_lo NULL = (0, 0), or a wide centre, never both); bits as there.
 * The arrays are fr_escape_rows_de's: all three required, y0 == y1 a no-op that needs no device.  Orbits and tables are the
 * context's caches, shared with the PT and BLA-PT calls (fr_debug_bla_cache shows a table served).  With profiling on,
 * fr_last_kernel_name reports escape_bla_de_kernel. */
int fr_escape_rows_de_pt_bla_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                                    uint32_t y1, void *d_z, void *d_iters, void *d_der, void *hip_stream);
int fr_escape_rows_de_pt_bla(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int bits, uint32_t y0,
                             uint32_t y1, double *z, uint32_t *iters, double *der);
/* DE ON SCALED PT (defined at fr_precision above): rows [y0, y1) with their SCALED derivatives u = d 2^-e on the SCALED PT road;
 * centre (required) and bits (-1: the plain scaled loop, 0 or 24 .. 53: the table) as the fr_*_pt_scaled calls take them.  The
 * arrays are fr_escape_rows_de's: all three required, y0 == y1 a no-op that needs no device.  z and iters are
 * fr_escape_rows_pt_scaled's bit for bit.  Orbits and tables are the context's caches, shared with the fr_*_pt_scaled calls of
 * the same view and bits (fr_debug_bla_cache shows a table served).  With profiling on, fr_last_kernel_name reports
 * escape_pt_scaled_de_kernel / escape_bla_scaled_de_kernel. */
int fr_escape_rows_de_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, void *d_z,
                                       void *d_iters, void *d_der, void *hip_stream);
int fr_escape_rows_de_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, uint32_t y0, uint32_t y1, double *z,
                                uint32_t *iters, double *der);
/* The scaled view cfg_v of DE ON SCALED PT: *view = *cfg with scale = (scale.re * Sinv, scale.im * Sinv), both exact.  The
 * distance and the shading of a scaled DE render are DE's own calls run on it (fr_distance_rows(_device),
 * fr_colour_de_rows_device, fr_colour_de_rgb8, fr_colour_de_rows_ss_device).  Host only; `view` may alias `cfg`.  Refuses what
 * SCALED PT's rules about the scale refuse: a NULL argument, a scale that is not finite, |scale| < 2^-64 on an axis, min |scale| <
 * 2^-32 max |scale|. */
int fr_de_scaled_view(const fr_config *cfg, fr_config *view);
/* RESUMABLE DE (defined at fr_precision above): a kept DE view answers an iterations change in place, derivative included.
 *
 * The F64 road: raise the cap of the (z, iters, der) that fr_escape_rows_de(_device) wrote, N = from_iterations -> M =
 * cfg->iterations, cfg_N = cfg with iterations = N:
 *   Precondition: the arrays hold what fr_escape_rows_de_device(cfg_N, FR_PRECISION_F64, NULL, y0, y1, ...) writes.
 *   Result: after the call they hold what the same call writes for cfg, bit for bit in all three arrays (z and iters are then
 *   also fr_escape_rows_device's at M).
 *   A pixel with iters[k] != N is finished: only that word is read; its z and der are neither loaded nor written.  Values of
 *   iters[k] above N are foreign data and are left alone like finished pixels.
 * The library CANNOT check the precondition, and the call is not idempotent (in arrays that already hold cap M, iters[k] == N
 * means "escaped at step N").  Domain (else FR_ERR_INVALID_ARGUMENT, before any device work): precision FR_PRECISION_F64 —
 * FR_PRECISION_PT is refused with a message that names fr_escape_extend_de_pt, everything else with DE's scope message; limit
 * <= 2^20; M >= N — M == N is a legal no-op that needs no device, as y0 == y1 is; all three arrays, z and der 8-byte aligned,
 * iters 4-byte aligned (y0 == y1 needs none).  An algorithm without orbits: nothing is done.  The _device form is asynchronous
 * on hip_stream, allocates nothing and takes no lock; the host form uploads, launches, downloads and synchronises as
 * fr_escape_extend does.  With profiling on, fr_last_kernel_name reports escape_extend_de_kernel. */
int fr_escape_extend_de_device(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, uint32_t from_iterations, void *d_z,
                               void *d_iters, void *d_der, void *hip_stream);
int fr_escape_extend_de(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, uint32_t from_iterations, double *z,
                        uint32_t *iters, double *der);
/* PT.  One road for both centres, as the fr_*_pt_bla calls take them: `centre` non-NULL selects WIDE PT's orbits and domain
 * (pos_lo must then be NULL and cfg->pos is not read), otherwise the centre is PT's (cfg->pos, pos_lo), pos_lo NULL = (0, 0).
 * fr_escape_rows_de_pt_state(_device): rows [y0, y1) with their DE state: z, dz, der 2 doubles per pixel (8-byte aligned),
 * iters, m one uint32 (4-byte aligned), all five required (y0 == y1 needs none and no device), k = (y - y0) * width + x.
 * z, iters, der are fr_escape_rows_de's (PT), dz and m fr_escape_rows_pt_state's, bit for bit.
 * fr_escape_extend_de_pt(_device): raise the cap of that state IN PLACE, N = from_iterations -> M = cfg->iterations, with
 * fr_escape_extend_pt's contract: the precondition (the arrays hold the state render of cfg_N) cannot be checked — arrays from
 * another view or cap are continued as if they were this one's, an index m beyond the orbit is brought inside it, nothing
 * more; the call is not idempotent; a pixel with iters[k] != N has only that word read and nothing of it loaded or written,
 * values above N included; M == N and y0 == y1 are no-ops that need no device; M < N is refused; an algorithm without orbits:
 * nothing is done.  Every refusal happens before any device work.
 * The calls use the context's orbit cache: a DE state render, a DE render and a PT render of one view share one orbit, and an
 * extension continues the orbit of the lower cap instead of recomputing it (fr_debug_pt_orbit_cache shows it).  The _device
 * forms allocate nothing.  With profiling on, fr_last_kernel_name reports escape_pt_de_state_kernel /
 * escape_extend_pt_de_kernel. */
int fr_escape_rows_de_pt_state_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, uint32_t y0,
                                      uint32_t y1, void *d_z, void *d_iters, void *d_dz, void *d_m, void *d_der, void *hip_stream);
int fr_escape_rows_de_pt_state(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                               double *z, uint32_t *iters, double *dz, uint32_t *m, double *der);
int fr_escape_extend_de_pt_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, uint32_t y0,
                                  uint32_t y1, uint32_t from_iterations, void *d_z, void *d_iters, void *d_dz, void *d_m, void *d_der,
                                  void *hip_stream);
int fr_escape_extend_de_pt(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                           uint32_t from_iterations, double *z, uint32_t *iters, double *dz, uint32_t *m, double *der);
/* RESUMABLE SCALED DE (defined at fr_precision above): a GUI keeps a DE view past 2^440 as (z, iters, w, m, der) in DEVICE memory
 * — 56 bytes per pixel — and answers an iterations change with fr_escape_extend_de_pt_scaled_device; the distance and the shading
 * are DE's calls over (z, iters, der) on the scaled view (fr_de_scaled_view).  The calls are the plain scaled loop's and take no
 * bits; `centre` is required.  Each is the counterpart of the fr_*_de_pt_state / fr_escape_extend_de_pt call it is named after,
 * with d_w / w where that one has d_dz / dz: the same buffers, alignment and asynchrony on `hip_stream`, nothing allocated by the
 * _device forms, and fr_escape_extend_pt_scaled's contract for the extension — the precondition (the arrays hold the state
 * render of cfg_N) cannot be checked; arrays from another view or cap are continued as if they were this one's, an index m beyond
 * the orbit is brought inside it, nothing more; the call is not idempotent; a pixel with iters[k] != N has only that word read
 * and nothing of it loaded or written, values above N included; M == N and y0 == y1 are no-ops that need no device; M < N is
 * refused; an algorithm without orbits: the render writes zeros into all five arrays, the extension does nothing.  Every refusal
 * happens before any device work.  z, iters and der are fr_escape_rows_de_pt_scaled's with bits = -1, w and m
 * fr_escape_rows_pt_scaled_state's, bit for bit.
 * The orbit is the shared slot's: a scaled DE state call serves and is served by every other scaled or wide call of the view, and
 * an extension computes only the missing orbit entries (fr_debug_pt_orbit_cache shows it).  The host forms go through the
 * context's scratch: upload (extension), launch, download, synchronise.  With profiling on, fr_last_kernel_name reports
 * escape_pt_scaled_de_state_kernel / escape_extend_pt_scaled_de_kernel. */
int fr_escape_rows_de_pt_scaled_state_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, void *d_z,
                                             void *d_iters, void *d_w, void *d_m, void *d_der, void *hip_stream);
int fr_escape_rows_de_pt_scaled_state(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, double *z,
                                      uint32_t *iters, double *w, uint32_t *m, double *der);
int fr_escape_extend_de_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1,
                                         uint32_t from_iterations, void *d_z, void *d_iters, void *d_w, void *d_m, void *d_der,
                                         void *hip_stream);
int fr_escape_extend_de_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, uint32_t y0, uint32_t y1, uint32_t from_iterations,
                                  double *z, uint32_t *iters, double *w, uint32_t *m, double *der);
/* D of n stored results, one double per pixel (8-byte aligned).  Reads only height, scale and iterations from cfg.  n <= 2^40;
 * n == 0 needs no device. */
int fr_distance_rows_device(const fr_config *cfg, const void *d_z, const void *d_iters, const void *d_der, size_t n, void *d_out,
                            void *hip_stream);
int fr_distance_rows(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, size_t n, double *out);
/* The colour map with distance shading over n stored results: channels 3 (r,g,b at any alignment) or 4 (r,g,b,255; d_out
 * 4-byte aligned), channels * n bytes.  thickness in pixels, finite, in [0, 2^20]; 0 = fr_colour_rows_device's bytes. */
int fr_colour_de_rows_device(const fr_config *cfg, const void *d_z, const void *d_iters, const void *d_der, size_t n,
                             double thickness, int channels, void *d_out, void *hip_stream);
/* the same over HOST arrays into packed r,g,b (upload, colour, download, synchronise: as fr_colour_rgb8) */
int fr_colour_de_rgb8(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, size_t n, double thickness,
                      uint8_t *out, size_t out_len);

/* SUPERSAMPLED DE (defined at fr_precision above).
 *
 * A KEPT anti-aliased DE view is a kept DE view of cfg_s: (z, iters, der) of the s times larger image in DEVICE memory, s * rows
 * rows of s * width samples, k = Y * (s * width) + X, 36 * s * s bytes per output pixel, written by any fr_escape_rows_de*_device
 * call for cfg_s.  fr_colour_de_rows_ss_device colours, shades and filters it in ONE kernel (colour_de_filter_kernel), with no
 * RGB image of cfg_s in between: thickness and exposure are a recolour.  DEFINITION:
 *   out = fr_box_filter_rgb8(fr_colour_de_rows(cfg_s, z, iters, der, n = s*s * width * rows, thickness * s), width, rows, s, channels),
 * byte for byte.  cfg is the OUTPUT image's config: cfg->height is the whole image's height (`rows` may be fewer: a row range of
 * the view), `width` the output width; cfg contributes what the colour map reads plus height, scale and iterations.  s = 1 is
 * fr_colour_de_rows_device.  An algorithm without orbits gives black.
 * Domain: s in 1 .. FR_SS_MAX with s * width, s * rows and s * cfg->height in 32 bits; thickness finite, 0 <= thickness * s <=
 * 2^20; channels 3 or 4 (RGBA output 4-byte aligned); d_z and d_der 8-byte aligned, d_iters 4-byte aligned; out_len >= channels *
 * width * rows (FR_ERR_BUFFER_TOO_SMALL); an empty output (width or rows 0) is a no-op without a device.  The device form is
 * asynchronous on `hip_stream`, allocates nothing and takes no lock.  fr_colour_de_ss_rgb8: the same over HOST arrays (upload to
 * context scratch, launch, download, synchronise, as fr_colour_de_rgb8 does). */
int fr_colour_de_rows_ss_device(const fr_config *cfg, const void *d_z, const void *d_iters, const void *d_der, uint32_t width,
                                uint32_t rows, uint32_t supersample, double thickness, int channels, void *d_out, size_t out_len,
                                void *hip_stream);
int fr_colour_de_ss_rgb8(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, uint32_t width, uint32_t rows,
                         uint32_t supersample, double thickness, int channels, uint8_t *out, size_t out_len);
/* Workspace of fr_render_rows_ss_de_device for rows [y0, y1): rows [s*y0, s*y1) of cfg_s are rendered in bands by
 * fr_ss_workspace_bytes' rule at 36 bytes per sample (36 * s * width bytes a source row): *min_bytes = one band of 8 * s source
 * rows (or all the rows if there are fewer), *best_bytes = the whole range, at most 1 GiB (never under *min_bytes); any length
 * from *min_bytes up is accepted and used, Bmax, nb and B as there.  Unlike the RGB road, s = 1 needs a workspace too: the arrays
 * must live somewhere.  LAYOUT: a band of n samples lies at d_work as z (16 n bytes) | der (16 n) | iters (4 n), each array as
 * the DE calls write it; d_work must be 8-byte aligned.  Either pointer may be NULL.  No device needed. */
int fr_ss_de_workspace_bytes(const fr_config *cfg, uint32_t supersample, uint32_t y0, uint32_t y1, size_t *min_bytes,
                             size_t *best_bytes);
/* Rows [y0, y1) of the SUPERSAMPLED DE image as r,g,b (channels 3) or r,g,b,255 (channels 4; d_out 4-byte aligned) into DEVICE
 * memory, asynchronously on `hip_stream`: band by band, the road's DE row launch into the workspace, then the fused kernel into
 * the band's place in d_out; the image of cfg_s never exists whole (a 3840 x 2160 frame at s = 4 would be 4.8 GB of arrays).
 * precision: FR_PRECISION_F64 (road FR_PT_ROAD_PLAIN, pos_lo NULL, centre NULL, bits 0) or FR_PRECISION_PT (road
 * FR_PT_ROAD_PLAIN with bits 0, or FR_PT_ROAD_BLA with bits 0 or 24 .. 53; pos_lo or centre or neither, never both;
 * FR_PT_ROAD_SCALED is refused by name).  The caller lends d_work (work_len bytes, 8-byte aligned) until the work queued on the
 * stream has finished; work_len under *min_bytes or a short out_len give FR_ERR_BUFFER_TOO_SMALL; y0 == y1 is a no-op without a
 * device.  The library allocates nothing and takes no lock beyond what the road's plain device call takes (the orbit / table
 * cache): the orbit — and for BLA the table — is computed and uploaded by the first band and served to the others
 * (fr_debug_pt_orbit_cache, fr_debug_bla_cache).  With profiling on, fr_last_kernel_name reports the road's DE kernel and
 * fr_last_kernel_ms the span from the first band's kernel to the last filter. */
int fr_render_rows_ss_de_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                int bits, double thickness, uint32_t supersample, uint32_t y0, uint32_t y1, int channels, void *d_out,
                                size_t out_len, void *d_work, size_t work_len, void *hip_stream);
/* The same into a HOST buffer of at least channels*width*(y1-y0) bytes: the workspace (at most 256 MiB) and the result live in
 * the context's scratch; the small image leaves the device in one copy. */
int fr_render_rows_ss_de(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                         double thickness, uint32_t supersample, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len);
/* SUPERSAMPLED SCALED DE (defined at fr_precision above): fr_render_rows_ss_de(_device) on DE ON SCALED PT's road.  `centre` is
 * required; bits: -1 = the plain scaled loop, 0 = FR_BLA_DEFAULT_BITS, else 24 .. 53.  Buffers, workspace (fr_ss_de_workspace_bytes,
 * 36 bytes per sample, its layout), alignment, asynchrony and error codes are fr_render_rows_ss_de_device's; the orbit — and
 * with a table the table — is computed and uploaded by the first band and served to the others.  With profiling on,
 * fr_last_kernel_name reports escape_pt_scaled_de_kernel / escape_bla_scaled_de_kernel and fr_last_kernel_ms the span from the first
 * band's kernel to the last filter.  The host form uses the context's scratch (workspace at most 256 MiB). */
int fr_render_rows_ss_de_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness,
                                          uint32_t supersample, uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len,
                                          void *d_work, size_t work_len, void *hip_stream);
int fr_render_rows_ss_de_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness, uint32_t supersample,
                                   uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len);

/* ---- adaptive supersampling: all s*s samples only at edge pixels ----------------------------------------------------- */

/* ADAPTIVE SUPERSAMPLING (fr_render_rows_ss_adaptive(_device) below).  Supersampling renders s*s samples of every output
 * pixel; most pixels lie in smooth regions, where one sample is the filtered average to within a grey level.  DEFINITION, for
 * supersample = s, 1 <= s <= FR_SS_MAX, and an integer threshold t, -1 <= t <= 255:
 *   cfg_s  = cfg with width * s and height * s, every other field unchanged;
 *   H      = the bytes of the road's plain render of cfg_s.  The roads are those of fr_render_rows_ss_de_device's argument rule
 *            plus FR_PT_ROAD_SCALED: FR_PRECISION_F64 (road PLAIN, no pos_lo, no centre, bits 0); FR_PRECISION_PT with
 *            FR_PT_ROAD_PLAIN (pos_lo, a wide centre or neither; bits 0), FR_PT_ROAD_BLA (pos_lo / centre as BLA-PT takes them,
 *            bits 0 or 24 .. 53) or FR_PT_ROAD_SCALED (centre required, pos_lo NULL, bits -1, 0 or 24 .. 53).  BLA-PT's D and
 *            SCALED PT's Dw are taken over the whole image of cfg_s, as the supersampled deep roads define;
 *   p      = floor(s / 2); the PROBE of output pixel (X, Y) is P(X, Y, c) = H(s*X + p, s*Y + p, c);
 *   F(X, Y, c) = (sum over j < s, i < s of H(s*X + i, s*Y + j, c) + floor(s*s / 2)) / (s*s), integer and truncating: the box
 *            filter of "supersampled rendering";
 *   edge(X, Y) holds when t < 0, and when a neighbour (X', Y') != (X, Y) exists with |X' - X| <= 1 and |Y' - Y| <= 1,
 *            0 <= X' < width and 0 <= Y' < height OF THE IMAGE (not of the call's rows), and a channel c with
 *            |P(X, Y, c) - P(X', Y', c)| > t;
 *   out(X, Y, c) = edge(X, Y) ? F(X, Y, c) : P(X, Y, c); with 4 channels alpha is 255;
 *   refined = the number of edge pixels in rows [y0, y1).
 * An algorithm without orbits gives black and refined = 0.  Consequences: t = -1 gives the bytes of fr_render_rows_ss /
 * fr_render_rows_ss_pt; t = 255 gives the probe image; s = 1 is the road's plain render for every t; any split of [0, height)
 * into row pieces gives the whole image's bytes and the same total refined.
 * A non-edge pixel's interior samples are NEVER LOOKED AT: a feature smaller than a pixel inside a flat neighbourhood is
 * missed.  Distance shading (SUPERSAMPLED DE) is the tool for that.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message that names the argument, before any device work): s in 1 .. FR_SS_MAX;
 * s * width and s * height fit in 32 bits; threshold in -1 .. 255; channels 3 or 4; the road's own domain ON cfg_s with the
 * argument rules above; width * (y1 - y0) < 2^32; d_work and a non-NULL d_refined 8-byte aligned; RGBA output 4-byte aligned.
 * FR_PRECISION_F32 and FR_PRECISION_DD are refused by name.  A work_len under the workspace size or a short out_len give
 * FR_ERR_BUFFER_TOO_SMALL.  y0 == y1 is a no-op that needs no device and no buffer.
 * Workspace: ONE size per row range, no banding — a caller with less memory calls by row pieces, which the definition makes
 * exact.  It holds the probe colours of rows [ya, yb) = [max(y0 - 1, 0), min(y1 + 1, height)), 3 bytes each, rounded up to 8
 * bytes; a uint32 list of at most width * (y1 - y0) pixel indices, rounded up to 8 bytes; and two 64-bit counters, the count
 * and the claim cursor, which every call zeroes on the stream:
 *   bytes = ceil8(3 * width * (yb - ya)) + ceil8(4 * width * (y1 - y0)) + 16        (0 for an empty range or width 0).
 * The device form is asynchronous on `hip_stream`: no host synchronisation (the PT roads: apart from computing and uploading
 * the view's orbit and table when the context does not hold them yet, as their plain device calls do), no allocation, and
 * re-entrant as fr_render_rows_ss_device is; d_refined (device memory, may be NULL) receives the count as a uint64 behind the
 * last kernel.  The F64 road makes one kernel choice for the call, by name and size: it takes no view sample.  The host form
 * uses the context's scratch; above the host roads' 256 MiB workspace cap it splits the range into row pieces itself.  With
 * profiling on, fr_last_kernel_name reports the last kernel of the call (ss_refine_*_kernel, or ss_mark_kernel when nothing is
 * refined) and fr_last_kernel_ms the span of the whole call. */
int fr_ss_adaptive_workspace_bytes(const fr_config *cfg, uint32_t supersample, uint32_t y0, uint32_t y1, size_t *bytes);
int fr_render_rows_ss_adaptive_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                      int bits, uint32_t supersample, int threshold, uint32_t y0, uint32_t y1, int channels, void *d_out,
                                      size_t out_len, void *d_work, size_t work_len, void *d_refined /* uint64 on the device, may be NULL */,
                                      void *hip_stream);
int fr_render_rows_ss_adaptive(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                               uint32_t supersample, int threshold, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len,
                               uint64_t *refined /* may be NULL */);
/* Test hook: the refine kernels' grid in workgroups of 4 waves; 0 = the default (it fills the device, capped by the most work
 * the rows can hold).  The output does not depend on it. */
int fr_debug_ss_adaptive_grid(uint32_t workgroups);
/* Test hook: the cap in bytes on the workspace that the host forms of the supersampled renders (fr_render_rows_ss, _ss_pt, _ss_de,
 * _ss_de_pt_scaled, _ss_adaptive, _ss_adaptive_de) reserve in the context's scratch; 0 = the default 256 MiB, any other value
 * must be a multiple of 8.  A banded call never goes below its min_bytes and an adaptive call never below one row a piece.  The
 * output does not depend on it. */
int fr_debug_ss_host_work_cap(size_t bytes);

/* ADAPTIVE SUPERSAMPLED DE (fr_render_rows_ss_adaptive_de(_device) below): ADAPTIVE SUPERSAMPLING and SUPERSAMPLED DE combined.
 * The adaptive call never looks at a non-edge pixel's interior samples; with distance estimation the probe KNOWS what it did not
 * sample: its exterior distance D says how far the set is, and a pixel whose probe is closer to the set than a caller-chosen
 * reach is refined whatever its neighbours look like.  DEFINITION, for supersample = s, 1 <= s <= FR_SS_MAX, a thickness T in
 * output pixels, an integer threshold t, -1 <= t <= 255, and a reach R in output pixels:
 *   cfg_s, (z, iters, der), Ts = T * (double)s and H are exactly those of SUPERSAMPLED DE: the road's DE render of cfg_s,
 *            coloured and shaded by fr_colour_de_rows_device(cfg_s, ..., Ts, 3);
 *   Dist(x, y) = D of "DE" for sample (x, y) of cfg_s: fr_distance_rows on cfg_s, in sample pixels, with the last factor
 *            (double)(s * height) * min(|scale.re|, |scale.im|);
 *   Rs     = R * (double)s, one f64 product;
 *   p      = floor(s / 2); the probe colour is P(X, Y, c) = H(s*X + p, s*Y + p, c), the probe distance Dp(X, Y) =
 *            Dist(s*X + p, s*Y + p), the probe index ip(X, Y) = iters(s*X + p, s*Y + p);
 *   F      = the integer box filter of "supersampled rendering", as in ADAPTIVE SUPERSAMPLING;
 *   near(X, Y) holds when ip(X, Y) < iterations and Dp(X, Y) < Rs: a capped probe is never near; an escaped probe with D = 0 (an
 *            overflowed derivative) is near whenever Rs > 0; R = 0 makes near false everywhere;
 *   edge(X, Y) holds when t < 0, or when ADAPTIVE SUPERSAMPLING's neighbour rule on P holds (8 neighbours inside the IMAGE, some
 *            channel differing by more than t), or when near(X, Y) holds;
 *   out(X, Y, c) = edge(X, Y) ? F(X, Y, c) : P(X, Y, c); with 4 channels alpha is 255;
 *   refined = the number of edge pixels in rows [y0, y1).
 * An algorithm without orbits gives black and refined = 0.  Consequences: t = -1 gives the bytes of fr_render_rows_ss_de for
 * every R (it is slower than that call: use that call); t = 255 with R = 0 gives the probe image; R = 0 is the colour rule on the
 * shaded bytes; s = 1 is the road's DE render followed by fr_colour_de_rows_device(cfg, ..., T, channels) for every t and R;
 * T = 0 with R = 0 gives fr_render_rows_ss_adaptive's bytes and count on the same road; any split of [0, height) into row pieces
 * gives the whole image's bytes and the same total refined (near reads the pixel's own probe only).
 * Roads: fr_render_rows_ss_de_device's argument rule — FR_PRECISION_F64 (road FR_PT_ROAD_PLAIN, pos_lo NULL, centre NULL, bits
 * 0) or FR_PRECISION_PT (road FR_PT_ROAD_PLAIN with bits 0, or FR_PT_ROAD_BLA with bits 0 or 24 .. 53 and D over the whole image
 * of cfg_s; pos_lo or centre or neither, never both); FR_PT_ROAD_SCALED is refused by name, as are FR_PRECISION_F32 and
 * FR_PRECISION_DD.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message that names the argument, before any device work): ADAPTIVE SUPERSAMPLING's
 * and SUPERSAMPLED DE's, plus reach finite with 0 <= R * s <= 2^20 and thickness finite with 0 <= T * s <= 2^20.  A work_len under
 * the workspace size or a short out_len give FR_ERR_BUFFER_TOO_SMALL.  y0 == y1 is a no-op that needs no device and no buffer.
 * Workspace: ONE size per row range, no banding.  With [ya, yb) = [max(y0 - 1, 0), min(y1 + 1, height)) and n = width * (yb - ya)
 * it holds, every array 8-byte aligned and in this order, the probe's z (16 n bytes), der (16 n), iters (ceil8(4 n)) and colours
 * (ceil8(3 n)), the edge list (ceil8(4 * width * (y1 - y0))) and two 64-bit counters:
 *   bytes = 32 n + ceil8(4 n) + ceil8(3 n) + ceil8(4 * width * (y1 - y0)) + 16        (0 for an empty range or width 0).
 * The device form is asynchronous on `hip_stream`: no host synchronisation (the PT roads: apart from computing and uploading the
 * view's orbit and table when the context does not hold them yet, as their plain device calls do), no allocation, re-entrant;
 * d_refined (device memory, may be NULL) receives the count as a uint64 behind the last kernel.  The host form uses the
 * context's scratch; above the host roads' 256 MiB workspace cap it splits the range into row pieces itself.  With profiling on,
 * fr_last_kernel_name reports the last kernel of the call (ss_refine_de_f64_kernel, ss_refine_de_pt_kernel or
 * ss_refine_de_bla_kernel, or ss_mark_de_kernel when no refine pass runs) and fr_last_kernel_ms the span of the whole call.
 * fr_debug_ss_adaptive_grid sets the grid of these refine kernels too.  FR_PT_ROAD_SCALED is out of scope of THESE calls; ADAPTIVE
 * SUPERSAMPLED SCALED DE below has calls of its own. */
int fr_ss_adaptive_de_workspace_bytes(const fr_config *cfg, uint32_t supersample, uint32_t y0, uint32_t y1, size_t *bytes);
int fr_render_rows_ss_adaptive_de_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre,
                                         int road, int bits, double thickness, uint32_t supersample, int threshold, double reach,
                                         uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work, size_t work_len,
                                         void *d_refined /* uint64 on the device, may be NULL */, void *hip_stream);
int fr_render_rows_ss_adaptive_de(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                  int bits, double thickness, uint32_t supersample, int threshold, double reach, uint32_t y0, uint32_t y1,
                                  int channels, uint8_t *out, size_t out_len, uint64_t *refined /* may be NULL */);

/* ADAPTIVE SUPERSAMPLED SCALED DE (fr_render_rows_ss_adaptive_de_pt_scaled(_device) below): ADAPTIVE SUPERSAMPLED DE past a scale of
 * 2^440, on DE ON SCALED PT's road, with its own calls; fr_render_rows_ss_adaptive_de keeps refusing FR_PT_ROAD_SCALED.  It is
 * ADAPTIVE SUPERSAMPLED DE word for word, with its inputs taken from the scaled road as SUPERSAMPLED SCALED DE takes them.
 * DEFINITION, for supersample = s, 1 <= s <= FR_SS_MAX, a thickness T in output pixels, an integer threshold t, -1 <= t <= 255, a
 * reach R in output pixels, bits in {-1, 0, 24 .. 53} and a wide centre, which is REQUIRED:
 *   cfg_s  = cfg with width * s and height * s, every other field unchanged;
 *   (z, iters, u) = fr_escape_rows_de_pt_scaled(cfg_s, centre, bits, ...), bit for bit; its Dw is taken over the whole image of
 *            cfg_s, as the supersampled deep roads define;
 *   cfg_sv = fr_de_scaled_view(cfg_s): cfg_s with scale = (sre, sim);
 *   Ts     = T * (double)s, one f64 product;
 *   H      = the bytes of fr_colour_de_rows_device(cfg_sv, z, iters, u, n, Ts, 3);
 *   Dist(x, y) = D of "DE" for sample (x, y): fr_distance_rows on cfg_sv, in sample pixels, with the last factor
 *            (double)(s * height) * min(|sre|, |sim|), one product;
 *   Rs, p, P, Dp, ip, F, near, edge, out and refined are exactly as ADAPTIVE SUPERSAMPLED DE states them, on this H, Dist and
 *            iters — the neighbour rule over the 8 neighbours inside the IMAGE and "a capped probe is never near" included.
 * An algorithm without orbits gives black and refined = 0.  Consequences:
 *   - t = -1 gives the bytes of fr_render_rows_ss_de_pt_scaled for every R (it is slower than that call: use that call);
 *   - t = 255 with R = 0 gives the probe image;
 *   - R = 0 is the colour rule on the shaded bytes;
 *   - s = 1 is fr_escape_rows_de_pt_scaled followed by fr_colour_de_rows_device(cfg_v, ..., T, channels) for every t and R;
 *   - T = 0 with R = 0 gives the bytes and the count of fr_render_rows_ss_adaptive with FR_PT_ROAD_SCALED and the same bits;
 *   - any split of [0, height) into row pieces gives the whole image's bytes and the same total refined;
 *   - inside WIDE PT's domain, where DE ON SCALED PT's claim 2 holds: with bits = -1 the bytes and the count equal
 *     fr_render_rows_ss_adaptive_de's on FR_PRECISION_PT, FR_PT_ROAD_PLAIN with the same wide centre; with bits >= 0 they equal
 *     FR_PT_ROAD_BLA's, subject to SCALED PT's own caveat about a pixel with |w| < 2^-53.
 * Domain (else FR_ERR_INVALID_ARGUMENT with a message that names the argument, before any device work): SUPERSAMPLED SCALED DE's
 * ON cfg_s (s in 1 .. FR_SS_MAX; s * width and s * height fit in 32 bits; DE ON SCALED PT's domain by the code the plain calls
 * run; T finite with 0 <= T * s <= 2^20; channels 3 or 4) and ADAPTIVE SUPERSAMPLED DE's rules: threshold in -1 .. 255; reach
 * finite with 0 <= R * s <= 2^20; width * (y1 - y0) < 2^32; d_work and a non-NULL d_refined 8-byte aligned; RGBA output 4-byte
 * aligned.  A work_len under the workspace size or a short out_len give FR_ERR_BUFFER_TOO_SMALL.  y0 == y1 is a no-op that needs
 * no device and no buffer.
 * Workspace: ADAPTIVE SUPERSAMPLED DE's layout and size — the probe's z, der (it holds u), iters and colours of rows [ya, yb),
 * then the edge list and the two counters; fr_ss_adaptive_de_workspace_bytes serves these calls unchanged.
 * Asynchrony, d_refined and the host form's split above the scratch cap are fr_render_rows_ss_adaptive_de(_device)'s.  With
 * profiling on, fr_last_kernel_name reports ss_refine_de_scaled_kernel, or ss_mark_de_kernel when no refine pass runs, and
 * fr_last_kernel_ms the span of the whole call.  fr_debug_ss_adaptive_grid sets the grid of this refine kernel too.  The _tf twins
 * (LINEAR-LIGHT SUPERSAMPLING below) replace F by that section's filter and nothing else.  No mark, colour or distance kernel is
 * added or changed.  The command line stays as it is. */
int fr_render_rows_ss_adaptive_de_pt_scaled_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness,
                                                   uint32_t supersample, int threshold, double reach, uint32_t y0, uint32_t y1, int channels,
                                                   void *d_out, size_t out_len, void *d_work, size_t work_len,
                                                   void *d_refined /* uint64 on the device, may be NULL */, void *hip_stream);
int fr_render_rows_ss_adaptive_de_pt_scaled(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness, uint32_t supersample,
                                            int threshold, double reach, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len,
                                            uint64_t *refined /* may be NULL */);

/* LINEAR-LIGHT SUPERSAMPLING (the _tf calls below).  Every supersampled call ends in the same reduction, the average of the s*s
 * sample BYTES.  The bytes are display-encoded (sRGB) values, so that average is not an average of light: one white sample
 * among black ones at s = 4 comes out at grey level 16 where the light's average is 71.  The _tf calls take a `transfer`
 * argument that chooses in which space the samples are averaged; FR_SS_TRANSFER_BYTES is the byte average of every call above. */
typedef enum fr_ss_transfer { FR_SS_TRANSFER_BYTES = 0, FR_SS_TRANSFER_SRGB = 1 } fr_ss_transfer;
/* DEFINITION.  Let f be the sRGB decoding function of IEC 61966-2-1:
 *   f(x) = x / 12.92 for x <= 0.04045,  f(x) = ((x + 0.055) / 1.055)^2.4 otherwise.
 * Decode table    L[v], v = 0 .. 255, uint16:  L[v] = floor(65535 * f(v / 255) + 1/2).
 * Threshold table T[k], k = 1 .. 255, uint16:  T[k] = ceil(65535 * f((k - 1/2) / 255)).
 * Both are committed as a generated include, csrc/fr_srgb_table.inc, beside its generator csrc/gen_srgb_table.py (`decimal` at
 * 100 digits).  No value is a tie: on the linear segment the argument is a rational that is never an integer or a half-integer,
 * elsewhere it is irrational.  THE COMMITTED NUMBERS ARE THE DEFINITION; the formulas say where they come from.  To pin them:
 *   L[0..4] = 0, 20, 40, 60, 80;  L[127] = 13909, L[128] = 14146;  L[254] = 64952, L[255] = 65535;
 *   T[1..4] = 10, 30, 50, 70;  T[128] = 14028, T[255] = 65244;
 *   SHA-256 of L as 256 little-endian uint16:      fdb7af3c01815a2118db8e50aac3c2304205ccc3f381f8976c588642c1aa60b6
 *   SHA-256 of T[1..255] as 255 little-endian uint16: f419ad49e531756005e2997106d1ec956b5c2839e9456ce3cb3df413d133d59a
 * Encode: E(m) for 0 <= m <= 65535 is the number of k in 1 .. 255 with m >= T[k].  Any search order gives the same value.
 * The filter, for FR_SS_TRANSFER_SRGB, with H the s-times-larger image exactly as each existing call defines it:
 *   n(X,Y,c)   = sum over j < s, i < s of L[ H(s*X+i, s*Y+j, c) ]          (at most 64 * 65535 < 2^22)
 *   m(X,Y,c)   = (n + floor(s*s/2)) / (s*s)     integer, truncating        (at most 65535)
 *   out(X,Y,c) = E(m)                           alpha stays 255 with 4 channels
 * For FR_SS_TRANSFER_BYTES, out is the existing byte formula, and every _tf call equals its existing twin byte for byte (the
 * twin IS the _tf call with FR_SS_TRANSFER_BYTES).  Any other transfer value is FR_ERR_INVALID_ARGUMENT with a message that
 * names the argument, before any device work and before any other argument is looked at.
 * Properties:
 *   - E(L[v]) = v for every v (DESIGN.md 3.31 proves it from the tables: L is strictly increasing and no L[v] is closer than 9
 *     to a threshold).  So s*s equal samples give that byte, and s = 1 is the plain render for either transfer;
 *   - E is non-decreasing;
 *   - adaptive forms: the probe P, the neighbour rule on P's bytes and the `near` rule are untouched; only F changes, to the
 *     filter above.  A non-edge pixel shows P in both transfers, so a flat region is identical in both; any split into row
 *     pieces still gives the whole image's bytes and the same `refined` count;
 *   - distance shading stays where it is, on the sample's bytes before the filter: H is unchanged.
 * The workspace of every call is unchanged: bands are still packed r,g,b (or the DE arrays), and fr_ss_workspace_bytes,
 * fr_ss_de_workspace_bytes and the two adaptive workspace calls serve the _tf calls as they are.  Each _tf call has its twin's
 * signature with `int transfer` behind `supersample`; domains, refusals and their messages, buffer rules, asynchrony and the
 * profiling reports are the twin's. */
int fr_box_filter_rgb8_tf(const uint8_t *src, uint32_t width, uint32_t rows, uint32_t supersample, int transfer, int channels, uint8_t *out,
                          size_t out_len);
int fr_box_filter_rgb8_tf_device(const void *d_src, uint32_t width, uint32_t rows, uint32_t supersample, int transfer, int channels,
                                 void *d_out, size_t out_len, void *hip_stream);
int fr_render_rows_ss_tf(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample, int transfer, uint32_t y0,
                         uint32_t y1, int channels, uint8_t *out, size_t out_len, const fr_render_opts *opts);
int fr_render_rows_ss_tf_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, uint32_t supersample, int transfer,
                                uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work, size_t work_len,
                                void *hip_stream, const fr_render_opts *opts);
int fr_render_rows_ss_pt_tf(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                            uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len);
int fr_render_rows_ss_pt_tf_device(const fr_config *cfg, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                                   uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len,
                                   void *d_work, size_t work_len, void *hip_stream);
int fr_colour_rows_ss_tf_device(const fr_config *cfg, const void *d_z, int z_width, const void *d_iters, uint32_t width, uint32_t rows,
                                uint32_t supersample, int transfer, int channels, void *d_out, size_t out_len, void *hip_stream);
int fr_colour_ss_rgb8_tf(const fr_config *cfg, const double *z, int z_width, const uint32_t *iters, uint32_t width, uint32_t rows,
                         uint32_t supersample, int transfer, int channels, uint8_t *out, size_t out_len);
int fr_colour_de_rows_ss_tf_device(const fr_config *cfg, const void *d_z, const void *d_iters, const void *d_der, uint32_t width,
                                   uint32_t rows, uint32_t supersample, int transfer, double thickness, int channels, void *d_out,
                                   size_t out_len, void *hip_stream);
int fr_colour_de_ss_rgb8_tf(const fr_config *cfg, const double *z, const uint32_t *iters, const double *der, uint32_t width, uint32_t rows,
                            uint32_t supersample, int transfer, double thickness, int channels, uint8_t *out, size_t out_len);
int fr_render_rows_ss_de_tf(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road, int bits,
                            double thickness, uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels, uint8_t *out,
                            size_t out_len);
int fr_render_rows_ss_de_tf_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                   int bits, double thickness, uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels,
                                   void *d_out, size_t out_len, void *d_work, size_t work_len, void *hip_stream);
int fr_render_rows_ss_de_pt_scaled_tf(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness, uint32_t supersample,
                                      int transfer, uint32_t y0, uint32_t y1, int channels, uint8_t *out, size_t out_len);
int fr_render_rows_ss_de_pt_scaled_tf_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness,
                                             uint32_t supersample, int transfer, uint32_t y0, uint32_t y1, int channels, void *d_out,
                                             size_t out_len, void *d_work, size_t work_len, void *hip_stream);
int fr_render_rows_ss_adaptive_tf(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                  int bits, uint32_t supersample, int transfer, int threshold, uint32_t y0, uint32_t y1, int channels,
                                  uint8_t *out, size_t out_len, uint64_t *refined /* may be NULL */);
int fr_render_rows_ss_adaptive_tf_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre,
                                         int road, int bits, uint32_t supersample, int transfer, int threshold, uint32_t y0, uint32_t y1,
                                         int channels, void *d_out, size_t out_len, void *d_work, size_t work_len,
                                         void *d_refined /* uint64 on the device, may be NULL */, void *hip_stream);
int fr_render_rows_ss_adaptive_de_tf(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre, int road,
                                     int bits, double thickness, uint32_t supersample, int transfer, int threshold, double reach, uint32_t y0,
                                     uint32_t y1, int channels, uint8_t *out, size_t out_len, uint64_t *refined /* may be NULL */);
int fr_render_rows_ss_adaptive_de_tf_device(const fr_config *cfg, int precision, const fr_imaginary *pos_lo, const fr_wide_centre *centre,
                                            int road, int bits, double thickness, uint32_t supersample, int transfer, int threshold,
                                            double reach, uint32_t y0, uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work,
                                            size_t work_len, void *d_refined /* uint64 on the device, may be NULL */, void *hip_stream);
int fr_render_rows_ss_adaptive_de_pt_scaled_tf(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness,
                                               uint32_t supersample, int transfer, int threshold, double reach, uint32_t y0, uint32_t y1,
                                               int channels, uint8_t *out, size_t out_len, uint64_t *refined /* may be NULL */);
int fr_render_rows_ss_adaptive_de_pt_scaled_tf_device(const fr_config *cfg, const fr_wide_centre *centre, int bits, double thickness,
                                                      uint32_t supersample, int transfer, int threshold, double reach, uint32_t y0,
                                                      uint32_t y1, int channels, void *d_out, size_t out_len, void *d_work, size_t work_len,
                                                      void *d_refined /* uint64 on the device, may be NULL */, void *hip_stream);
/* Host only, no device needed: pointers into the library's own copy of L (256 entries) and of T[1 .. 255] (255 entries, T[k] at
 * index k - 1), so a binding or a test reads the definition from the library itself.  Either argument may be NULL.  fr_ss_table
 * is `const uint16_t *`: the call is int fr_ss_transfer_tables(const uint16_t **decode256, const uint16_t **thresholds255). */
typedef const uint16_t *fr_ss_table;
int fr_ss_transfer_tables(fr_ss_table *decode256, fr_ss_table *thresholds255);

/* ---- measurement --------------------------------------------------------------------------- */

/* Exact sum of EXECUTED loop iterations over the pixels (x, y) with x % sx == 0, y % sy == 0 of
 * rows [y0, y1): a pixel that escapes at index i executed i+1, one that exhausts the cap executed
 * `iterations`.  Computed on the device. */
int fr_count_iterations(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, uint32_t sx,
                        uint32_t sy, uint64_t *total, uint64_t *pixels);

/* When enabled, device-pointer renders record HIP events around the escape+colour kernel on the
 * stream they are launched on; fr_last_kernel_ms() waits for that kernel and returns its
 * duration.  State is per calling thread. */
int fr_set_profiling(int enabled);
int fr_last_kernel_ms(float *ms);
/* Name of the render kernel the calling thread's last device-pointer render launched (profiling on),
 * e.g. "escape_strip_kernel<double, 7 tiles>": bench.py reports what actually ran. */
int fr_last_kernel_name(char *buf, size_t buf_len);

/* Kernel-variant selector for tuning studies and tests; every variant produces the same bytes.
 * 0 = default: strips of 8x8 tiles (one tile per workgroup under 8192 x 4096 pixels, seven from there up) unless the view's
 *     own statistics call for another kernel or strip length — see fr_set_dispatch_sampling; without statistics (the first
 *     frame of a GUI-sized view, sampling off): two passes (11) for Julia images of 4096^2 pixels and more with a cap of
 *     512 and more, strips otherwise;
 * 1, 2, 4 = the strip kernel with a fixed strip length of 1, 2, 4 tiles, 8 = of 7 tiles (the longest);
 * 9 = 7-tile strips with lane refill;
 * 10 = the work-queue kernel (persistent waves drawing 64x32-pixel patches from a device-wide counter, unchecked
 *      blocks of iterations, results finished and coloured 64 at a time; RGB renders of an escape-time algorithm
 *      whose loop plan allows the scaled form — otherwise it acts as 9);
 * 11 = two passes: 7-tile strips run every pixel through episodes of a few
 *      dozen iterations and colour what has escaped, tile by tile; a tile whose running lanes fall under a
 *      threshold hands them — position, iterations done, output position — to lists in device memory, which the
 *      persistent waves of a second kernel then finish.  Same conditions as 10 (otherwise it acts as 9).  The
 *      lists live in a context-owned ring of three buffers cut from one allocation: per entry 20 bytes (f32 Julia),
 *      28 (f64 Julia; f32 Mandelbrot), 44 (f64 Mandelbrot), one entry per eight pixels of the launch (at most 2^28
 *      entries) — C4 in f32: 671 MB per buffer, 2 GB for the ring.  The ring exists from the context's creation on
 *      for frames up to 3840 x 2160 (3 x 48 MiB, best effort) and is re-allocated only for a launch that needs more: the one
 *      allocation a device-pointer render can block on (~15 ms, once per size never seen before; other threads' renders that
 *      need no lists are not held up by it).  A list that is full costs speed only;
 * 12 = two passes with round 2's two kernels (kept for comparisons: tools/c4_ab.py);
 * 13 = the first pass of 11 alone: no tile is handed over (every lane finishes in place), no lists, no second kernel;
 * 14 = 11 with round 2's second-pass kernel behind this round's first pass (kept for comparisons);
 * 15 = 11 with the first pass in 4-tile strips, 16 = 13 in 4-tile strips (GUI-sized launches: four times as many
 *      workgroups to balance over the chip);
 * 6401, 3202, 1604, 808 = the 4-wave-workgroup kernel with a 64x1 / 32x2 / 16x4 / 8x8 per-wave
 * pixel footprint. */
int fr_set_tile(int tile);

/* The default dispatch (tile 0) chooses its kernel from the IMAGE: a sample of 16 x 16 tiles of the launch goes through the
 * plain loop (capped at 4096 iterations; ~20-70 us of device time) and reports the share of pixels still running at the cap
 * (`capped`), the share the two-pass render would hand over to its lists (`handed`), the lane-iterations that finishing those
 * in place would idle away as a share of the work (`waste`) and the mean iteration count.
 *   Launches of 131 072 tiles (4096 x 2048 pixels) and more — the sample is taken in FRONT of the first launch of a view,
 *   on a stream of the library's own, and the calling thread waits for it (~40 us): the ONE step of the device-pointer entry
 *   points that blocks.  Rule: capped >= 0.10 and waste < 0.01 -> strips; else handed >= 0.002 (or >= 4096 handed-over
 *   pixels with >= 128 iterations to go on average) -> two passes; else the first pass alone.
 *   (Launches under 524 288 tiles, 8192 x 4096, use the rule of the next paragraph instead.)
 *   Launches of 4096 .. 131 072 tiles — every frame the reference's GUI asks for (src/gui.rs:56-82) — NEVER block: the first
 *   frame of a view is dispatched by size as described under fr_set_tile, the sample is enqueued BEHIND its render, and the
 *   next frame of the same view is dispatched from the measured numbers.  Rule: capped < 0.001 and either mean < 16 with
 *   handed < 0.002 (orbits of a dozen iterations everywhere) or, from 100 000 tiles up, mean < 32 with waste < 1 -> the first
 *   pass alone (4- or 7-tile strips; 4-tile strips of the strip kernel for a Julia constant the scaled loop may not use);
 *   handed >= 0.05 and waste >= 2 (a Julia dust) from 60 000 tiles up in f64, 200 000 in f32 -> two passes; everything else
 *   -> one-tile strips.
 * A view is identified by the fields that determine orbits (algo, width, height, iterations, limit, pos, scale, julia_set),
 * the launch's rows and the precision: changing colours, exposure, smooth or inside keeps it.  The last 32 views are
 * remembered.  No sample is taken while `hip_stream` is being captured into a graph.  0 switches sampling off (dispatch
 * by algorithm and size only).  Same bytes either way. */
int fr_set_dispatch_sampling(int enabled);
/* Tool / test hook: the (blocking) sample of the whole image. out[0..5] = executed iterations, 64 x the sum of the tiles'
 * longest orbits, tiles, lanes at the sample's cap (min(iterations, 4096)), lanes the two-pass render's first-pass schedule
 * would hand over, lane-iterations that finishing those in place would waste; out[6] = out[0] / out[1], the useful-lane
 * fraction of one-tile-per-wave rendering; out[7] = iterations the handed-over lanes would still have to run. */
int fr_debug_sample_view(const fr_config *cfg, int precision, double out[8]);
/* Tool / test hook: what the default dispatch has on record for the view (cfg, rows [y0, y1), precision) as ONE launch:
 * *state = 0 nothing, 1 a non-blocking sample is in flight, 3 its totals have arrived (the next frame reads them), 2 decided; *choice = -1 none, 0 strips, 1 two passes, 2 the first
 * pass alone; *strip_tiles = the strip length it asks for (0 = by launch size).  Touches nothing. */
int fr_debug_view_choice(const fr_config *cfg, int precision, uint32_t y0, uint32_t y1, int *state, int *choice,
                         uint32_t *strip_tiles);

/* Policy of the lane-refilling kernels (tuning studies): an orbit episode may end early, so that
 * idle lanes get new pixels, once quit16/16 of its running lanes (work-queue kernel: of the wave's 64 lanes)
 * have finished and at least `minrun` iterations were done.  With tile 11 the two numbers steer its first pass
 * instead: `minrun` = the length of an episode (default 64), `quit16` x 4 = the running lanes a tile needs to stay
 * in the first pass for another episode (default 12: 48 lanes).  -1 = the kernel's own measured default.  Does
 * not affect results. */
int fr_set_refill_policy(int minrun, int quit16);

/* Exact periodicity shortcut, OFF by default.  When on, large images are rendered by the refilling
 * kernel and an orbit that returns BITWISE to a state it has already visited (the floating-point map
 * z -> z^2 + c is a deterministic function of the state, so it is then exactly periodic and can never
 * escape) is fast-forwarded to the iteration cap — (cap - k) mod d further steps — instead of being
 * iterated there.  Output bytes, escape indices and final positions are identical to the plain loop;
 * only the work differs, so bench.py's headline is measured with it off and reports the on-number
 * separately. */
int fr_set_cycle_shortcut(int enabled);

/* smooth == false renders look the outside colour up in an LDS-staged palette (one entry per
 * escape index, built once per call on the device) when iterations < 1280; 0 disables that and
 * computes the colour per pixel.  Same bytes either way (tests compare them). */
int fr_set_palette(int enabled);

/* Smooth colouring needs log2(log2(sqrt(dist)) / 2) per outside pixel (calc/src/lib.rs:222-223).  With
 * the filter on (default) the kernel first brackets that value with the hardware's f32 log and a
 * proven error bound, evaluates the rest of the colour map in f64 at both ends of the bracket and
 * keeps the bytes if they agree (the map is monotone); only pixels whose bracket straddles a byte
 * boundary take the full f64 software log2.  1 (default) first makes the same test in f32 arithmetic, with a
 * correspondingly wider window, and goes to f64 only for the waves that fail it; 2 = the f64 test only;
 * 0 = always the software log2.  Same bytes in all three (tests compare them). */
int fr_set_colour_filter(int enabled);

/* Orbit-loop selector for tuning studies and tests: -1 = automatic (default); 0 = the unscaled
 * loop with an escape check every iteration; 4 / 2 = the scaled loop that checks every 4th / 2nd
 * iteration, used only where it is provably bit-identical (otherwise the call still falls back to
 * 0).  In the four-iteration scaled loop and in the unscaled loop a wave whose lanes have all stayed quiet
 * (far inside the limit / none escaping) for 16 iterations goes on in speculative blocks of 16 unchecked
 * iterations that keep their start state in a second register set: one test at the block's end, the block
 * thrown away and re-run with checks if it fails (only where 16 <= limit^2 <= 2^1000 — f32: 2^100 —, every
 * |c| component <= limit^2 / 8 and the view's coordinates are finite: an orbit past the limit then grows
 * monotonically and passes the limit before anything overflows, so an escape inside a block cannot be
 * missed at its end; fr_debug_loop_plan shows the plan).
 * 5 = automatic without those speculative blocks (A/B).  Every mode produces the same bytes. */
int fr_set_loop_mode(int mode);
/* Tool / test hook, host arithmetic only (works without a device): the loop plan of (cfg, precision) as one launch
 * under the current selectors — *loop_mode = 0 / 2 / 4 as above, *skip_t = the squared distance under which escape
 * checks are skipped, *spec_quiet = iterations a wave must stay under it before it speculates (0 = never). */
int fr_debug_loop_plan(const fr_config *cfg, int precision, uint32_t *loop_mode, double *skip_t, uint32_t *spec_quiet);
/* The speculative blocks of the four-iteration scaled loop grow while a tile stays quiet: 16 iterations, doubling after
 * every block that passes its end test, up to `maxlen` (default 128; brought down to 16 * 2^k), and 16 for good once the
 * tile has thrown a block away.  Tool / test hook: sets `maxlen` for every later render of the process (0 = the
 * default, 16 = blocks of 16 only); every value produces the same bytes. */
int fr_debug_set_spec_maxlen(uint32_t maxlen);
/* Host arithmetic only, as fr_debug_loop_plan: *maxlen = the longest block the launch of (cfg, precision) would run
 * with — 0 wherever *spec_quiet is 0. */
int fr_debug_spec_maxlen(const fr_config *cfg, int precision, uint32_t *maxlen);

/* Test hook (not part of the reference surface): elementwise DEVICE arithmetic over host arrays —
 * which = 0: the kernels' software log2, 1: sqrt, 2: in[k] / in[(k+1) % n], 3: the `as u8` cast —
 * so tests can compare the device's roundings with the host's; which = 4: the colour filter's
 * bracket centre against the f64 nu over EVERY f32 bit pattern in [in[0], in[1]], out[0] = worst error;
 * which = 5: the packed form of the cast ((float)in[k] into byte 1 of the word 0xAABBCCDD, returned whole);
 * which = 6: the number of f32 bit patterns in [in[0], in[1]] on which the packed and the plain cast differ. */
int fr_debug_math(int which, const double *in, double *out, size_t n);
/* Tuning aid: a device buffer of 16 uint64 per persistent wave (8192 waves is enough) to which the waves of the
 * persistent kernels (tile 10; the second pass of 11 / 12 / 14) write their start / end times (100 MHz ticks) and
 * work counts (round 2's kernel also the cycles per phase); NULL turns it off. */
int fr_debug_set_queue_trace(void *d_trace);
/* Test aid: entries per survivor list of the two-pass render (tile 11); 0 = sized from the image.  A tiny
 * value makes the lists overflow, which the first pass absorbs by finishing those pixels itself. */
int fr_debug_set_two_pass_capacity(uint32_t entries_per_list);

#ifdef __cplusplus
}
#endif
#endif /* FRACTAL_HIP_H */
