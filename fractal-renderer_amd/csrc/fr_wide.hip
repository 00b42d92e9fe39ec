/*
 * fr_wide.hip — WIDE PT's host arithmetic (include/fractal_hip.h, "WIDE PT"): a view centre of up to 1016 bits and the
 * reference orbits iterated from it.  No device code: the orbits feed escape_pt_kernel, escape_pt_state_kernel and
 * escape_extend_pt_kernel (fr_pt.hip) as their stored f64 entries, exactly as the dd orbits do.
 *
 * A number is n little-endian uint64_t words in two's complement, value I / 2^F with F = 64 n - 8.  Products are schoolbook
 * limb products through unsigned __int128 on the magnitudes; the sign goes back on the exact 2n-word product, and the
 * arithmetic shift that follows is the floor of the definition.  tests/pt_wide_model.py restates all of it on Python
 * integers.
 */
#include <cmath>
#include <cstring>
#include <string>

#include "fr_ctx.h"
#include "fr_wide.h"

namespace {

typedef unsigned __int128 u128;
constexpr uint32_t kMaxWords = FR_WIDE_MAX_WORDS;

bool negative(const uint64_t *w, uint32_t n) { return (w[n - 1] >> 63) != 0; }

void negate(uint64_t *w, uint32_t n) {
    uint64_t carry = 1;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t v = ~w[i] + carry;
        carry = (carry && v == 0) ? 1 : 0;
        w[i] = v;
    }
}

void add_to(uint64_t *a, const uint64_t *b, uint32_t n) {
    uint64_t carry = 0;
    for (uint32_t i = 0; i < n; i++) {
        const u128 t = (u128)a[i] + b[i] + carry;
        a[i] = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
    }
}

void sub_from(uint64_t *a, const uint64_t *b, uint32_t n) {
    uint64_t borrow = 0;
    for (uint32_t i = 0; i < n; i++) {
        const u128 t = (u128)a[i] - b[i] - borrow;
        a[i] = (uint64_t)t;
        borrow = (uint64_t)(t >> 64) & 1u;
    }
}

/* |w| into m (the magnitude of -2^(64n-1) fits unsigned); returns the sign */
bool magnitude(const uint64_t *w, uint32_t n, uint64_t *m) {
    memcpy(m, w, n * sizeof(uint64_t));
    const bool neg = negative(w, n);
    if (neg) negate(m, n);
    return neg;
}

/* floor(P / 2^(F - extra)) of the signed 2n-word product P, n words of it (extra 0: mul, 1: mul2) */
void shift_product(const uint64_t *p, uint32_t n, unsigned extra, uint64_t *out) {
    const unsigned sh = 56 - extra;
    for (uint32_t i = 0; i < n; i++) out[i] = (p[i + n - 1] >> sh) | (p[i + n] << (64 - sh));
}

/* out = floor(2^extra a b / 2^F) */
void mul_floor(const uint64_t *a, const uint64_t *b, uint32_t n, unsigned extra, uint64_t *out) {
    uint64_t ma[kMaxWords], mb[kMaxWords], p[2 * kMaxWords];
    const bool neg = magnitude(a, n, ma) != magnitude(b, n, mb);
    memset(p, 0, 2 * n * sizeof(uint64_t));
    for (uint32_t i = 0; i < n; i++) {
        uint64_t carry = 0;
        for (uint32_t j = 0; j < n; j++) {
            const u128 t = (u128)ma[i] * mb[j] + p[i + j] + carry;
            p[i + j] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        p[i + n] = carry;
    }
    if (neg) negate(p, 2 * n);
    shift_product(p, n, extra, out);
}

/* out = floor(a a / 2^F): the off-diagonal limb products once, doubled, plus the diagonal */
void sqr_floor(const uint64_t *a, uint32_t n, uint64_t *out) {
    uint64_t m[kMaxWords], p[2 * kMaxWords];
    magnitude(a, n, m);
    memset(p, 0, 2 * n * sizeof(uint64_t));
    for (uint32_t i = 0; i < n; i++) {
        uint64_t carry = 0;
        for (uint32_t j = i + 1; j < n; j++) {
            const u128 t = (u128)m[i] * m[j] + p[i + j] + carry;
            p[i + j] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        p[i + n] = carry;
    }
    for (uint32_t i = 2 * n; i-- > 1;) p[i] = (p[i] << 1) | (p[i - 1] >> 63);
    p[0] <<= 1;
    uint64_t carry = 0;
    for (uint32_t i = 0; i < n; i++) {
        const u128 t = (u128)m[i] * m[i] + p[2 * i] + carry;
        p[2 * i] = (uint64_t)t;
        const u128 t2 = (t >> 64) + p[2 * i + 1];
        p[2 * i + 1] = (uint64_t)t2;
        carry = (uint64_t)(t2 >> 64);
    }
    shift_product(p, n, 0, out);
}

/* bit k of the magnitude m (n words) */
inline uint64_t bit(const uint64_t *m, uint32_t k) { return (m[k >> 6] >> (k & 63)) & 1u; }

/* the f64 nearest to I / 2^F, ties to even.  |value| < 2^7 and its lowest bit is 2^-1016 at the least: the result is a
 * normal number whatever the words hold. */
double to_f64(const uint64_t *w, uint32_t n) {
    uint64_t m[kMaxWords];
    const bool neg = magnitude(w, n, m);
    int top = (int)n - 1;
    while (top >= 0 && m[top] == 0) top--;
    if (top < 0) return 0.0;
    const int F = 64 * (int)n - 8;
    const uint32_t msb = 64u * (uint32_t)top + 63u - (uint32_t)__builtin_clzll(m[top]);
    double r;
    if (msb < 53) {
        r = std::ldexp((double)m[0], -F);
    } else {
        const uint32_t shift = msb - 52;
        const uint32_t word = shift >> 6, b = shift & 63;
        uint64_t sig = m[word] >> b;
        if (b && word + 1 < n) sig |= m[word + 1] << (64 - b);
        sig &= (1ull << 53) - 1;
        const uint64_t half = bit(m, shift - 1);
        bool sticky = false;
        for (uint32_t k = 0; k + 1 < shift && !sticky; k += 64) {
            const uint32_t left = shift - 1 - k; /* bits k .. shift - 2 are below the rounding bit */
            const uint64_t mask = left >= 64 ? ~0ull : ((1ull << left) - 1);
            sticky = (m[k >> 6] & mask) != 0;
        }
        if (half && (sticky || (sig & 1u))) sig++;
        r = std::ldexp((double)sig, (int)shift - F);
    }
    return neg ? -r : r;
}

/* floor(v 2^F) into w; v finite, |v| < 2^7 */
void from_f64(double v, uint64_t *w, uint32_t n) {
    memset(w, 0, n * sizeof(uint64_t));
    if (v == 0.0) return;
    int e;
    const double f = std::frexp(std::fabs(v), &e); /* |v| = sig 2^(e - 53) */
    const uint64_t sig = (uint64_t)std::ldexp(f, 53);
    const int shift = e - 53 + 64 * (int)n - 8;
    bool dropped = false;
    if (shift >= 0) {
        const uint32_t word = (uint32_t)shift >> 6, b = (uint32_t)shift & 63;
        w[word] = sig << b;
        if (b && word + 1 < n) w[word + 1] = sig >> (64 - b);
    } else if (shift > -64) {
        w[0] = sig >> -shift;
        dropped = (sig & ((1ull << -shift) - 1)) != 0;
    } else {
        dropped = true;
    }
    if (v < 0.0) { /* floor(-x) = -ceil(x) */
        if (dropped) {
            uint64_t one[kMaxWords] = {1};
            add_to(w, one, n);
        }
        negate(w, n);
    }
}

/* |value| <= 2 */
bool within_two(const uint64_t *w, uint32_t n) {
    const int64_t top = (int64_t)w[n - 1];
    if (top < 0) return top >= (int64_t)0xFE00000000000000ull;
    if (top < (int64_t)0x0200000000000000ll) return true;
    if (top > (int64_t)0x0200000000000000ll) return false;
    for (uint32_t i = 0; i + 1 < n; i++)
        if (w[i]) return false;
    return true;
}

int check_words(const uint64_t *w, uint32_t n) {
    if (n < 2 || n > kMaxWords) return fr::fail(FR_ERR_INVALID_ARGUMENT, "a wide number has 2 .. FR_WIDE_MAX_WORDS (16) words");
    if (!w) return fr::fail(FR_ERR_INVALID_ARGUMENT, "the words of a wide number are NULL");
    return FR_OK;
}

int out_of_range() { return fr::fail(FR_ERR_INVALID_ARGUMENT, "a wide number must stay within [-2, 2]"); }

/* ---- decimal strings: a magnitude of any length, base 2^64 ---- */

typedef std::vector<uint64_t> Big;

void big_mul_add(Big &b, uint64_t mul, uint64_t add) {
    uint64_t carry = add;
    for (uint64_t &x : b) {
        const u128 t = (u128)x * mul + carry;
        x = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
    }
    if (carry) b.push_back(carry);
}

/* b = floor(b / d); returns whether a remainder was left */
bool big_div(Big &b, uint64_t d) {
    u128 rem = 0;
    for (size_t i = b.size(); i-- > 0;) {
        const u128 t = (rem << 64) | b[i];
        b[i] = (uint64_t)(t / d);
        rem = t % d;
    }
    while (!b.empty() && b.back() == 0) b.pop_back();
    return rem != 0;
}

constexpr size_t kMaxDecimalLength = 8192;

}  // namespace

namespace fr {

void wide_key(const fr_wide_centre *centre, std::vector<uint64_t> &key) {
    const uint32_t n = centre->n_words;
    key.assign(1, n);
    key.insert(key.end(), centre->re, centre->re + n);
    key.insert(key.end(), centre->im, centre->im + n);
}

int check_pt_wide(const fr_config *cfg, const fr_wide_centre *centre, bool scaled) {
    const std::string name(scaled ? "SCALED PT: " : "FR_PRECISION_PT, wide centre: ");
    if (!cfg) return fail(FR_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (!centre) return fail(FR_ERR_INVALID_ARGUMENT, name + "centre is NULL");
    const uint32_t n = centre->n_words;
    if (n < 2 || n > kMaxWords) return fail(FR_ERR_INVALID_ARGUMENT, name + "n_words must lie in 2 .. FR_WIDE_MAX_WORDS (16)");
    if (!centre->re || !centre->im) return fail(FR_ERR_INVALID_ARGUMENT, name + "the centre's words are NULL");
    /* PT's domain on the fields that are read (cfg->pos is not) */
    const double fields[] = {cfg->limit,    cfg->stable_limit, cfg->scale.re,     cfg->scale.im,
                             cfg->exposure, cfg->color_weight, cfg->julia_set.re, cfg->julia_set.im};
    for (double v : fields)
        if (!std::isfinite(v)) return fail(FR_ERR_INVALID_ARGUMENT, name + "every field of the view must be finite");
    if (scaled && !(cfg->limit > 0.0 && cfg->limit <= 0x1p20))
        return fail(FR_ERR_INVALID_ARGUMENT, name + "limit must lie in (0, 2^20]: the scaled offset, at most about (limit^2 + 2) 2^e, "
                                                    "must stay finite");
    if (!(cfg->limit > 0.0 && cfg->limit <= 0x1p500)) return fail(FR_ERR_INVALID_ARGUMENT, name + "limit must lie in (0, 2^500]");
    if (cfg->iterations > FR_PT_MAX_ITERATIONS)
        return fail(FR_ERR_INVALID_ARGUMENT, name + "iterations must be <= FR_PT_MAX_ITERATIONS (2^24): the reference orbit takes "
                                                    "16 bytes per iteration");
    const double sre = std::fabs(cfg->scale.re), sim = std::fabs(cfg->scale.im);
    if (sre < 0x1p-64 || sim < 0x1p-64) return fail(FR_ERR_INVALID_ARGUMENT, name + "|scale| must be >= 2^-64 on both axes");
    if (scaled && (sre < sim ? sre : sim) < 0x1p-32 * (sre > sim ? sre : sim))
        return fail(FR_ERR_INVALID_ARGUMENT, name + "min |scale| must be >= 2^-32 max |scale| over the two axes");
    if (!scaled && (sre > 0x1p440 || sim > 0x1p440))
        return fail(FR_ERR_INVALID_ARGUMENT, name + "|scale| must be <= 2^440 on both axes (deeper views need a scaled pixel loop)");
    if (std::fabs(cfg->julia_set.re) > 2.0 || std::fabs(cfg->julia_set.im) > 2.0)
        return fail(FR_ERR_INVALID_ARGUMENT, name + "the components of julia_set must lie in [-2, 2]");
    if (!within_two(centre->re, n) || !within_two(centre->im, n))
        return fail(FR_ERR_INVALID_ARGUMENT, name + "the components of the centre must lie in [-2, 2]");
    int e;
    (void)std::frexp(sre > sim ? sre : sim, &e);
    if (64 * (int)n - 8 < e + 64)
        return fail(FR_ERR_INVALID_ARGUMENT, name + "the centre is too coarse for this scale: 64 n_words - 8 >= e + 64 is needed, "
                                                    "where max |scale| = f 2^e with 0.5 <= f < 1");
    return FR_OK;
}

void wide_reference_orbit(const fr_config *cfg, const fr_wide_centre *centre, int which, std::vector<double> &out, bool &ended,
                          WideTail &tail, const WideTail *from, uint32_t last) {
    const uint32_t n = centre->n_words;
    const bool julia = cfg->algo == 2;
    const uint32_t kmin = julia ? 1u : 2u;
    const uint32_t kmax = julia ? (cfg->iterations > 1 ? cfg->iterations : 1u) : cfg->iterations + 1u;
    uint64_t zr[kMaxWords] = {}, zi[kMaxWords] = {}, ar[kMaxWords], ai[kMaxWords], t[kMaxWords], u[kMaxWords];
    if (julia) { /* the constant added in a step: J, or C */
        from_f64(cfg->julia_set.re, ar, n);
        from_f64(cfg->julia_set.im, ai, n);
    } else {
        memcpy(ar, centre->re, n * sizeof(uint64_t));
        memcpy(ai, centre->im, n * sizeof(uint64_t));
    }
    if (julia && which == 0) {
        memcpy(zr, centre->re, n * sizeof(uint64_t));
        memcpy(zi, centre->im, n * sizeof(uint64_t));
    }
    bool stored = false; /* entry k is in the orbit already and has passed its tests */
    uint32_t k = 0;
    if (from) {
        if (last >= kmax) return; /* the caller keeps what it has */
        memcpy(zr, from->re.data(), n * sizeof(uint64_t));
        memcpy(zi, from->im.data(), n * sizeof(uint64_t));
        k = last, stored = true;
    }
    out.reserve(out.size() + 2 * ((size_t)(kmax - k) + 1));
    for (;; k++) {
        if (!stored) {
            const double re = to_f64(zr, n), im = to_f64(zi, n);
            out.push_back(re);
            out.push_back(im);
            ended = k >= kmin && re * re + im * im > 4.0;
            if (ended || k == kmax) break;
        }
        stored = false;
        if (!julia && k == 0) {
            memcpy(zr, ar, n * sizeof(uint64_t)); /* R_1 = C */
            memcpy(zi, ai, n * sizeof(uint64_t));
        } else {
            sqr_floor(zr, n, t);
            sqr_floor(zi, n, u);
            sub_from(t, u, n);
            add_to(t, ar, n);
            mul_floor(zr, zi, n, 1, u);
            add_to(u, ai, n);
            memcpy(zr, t, n * sizeof(uint64_t));
            memcpy(zi, u, n * sizeof(uint64_t));
        }
    }
    tail.re.assign(zr, zr + n);
    tail.im.assign(zi, zi + n);
}

}  // namespace fr

/* ---- the public helpers: host only ------------------------------------------------------------------------------- */

int fr_wide_from_double(double v, uint64_t *w, uint32_t n) {
    const int rc = check_words(w, n);
    if (rc != FR_OK) return rc;
    if (!std::isfinite(v)) return fr::fail(FR_ERR_INVALID_ARGUMENT, "fr_wide_from_double: the value is not finite");
    if (std::fabs(v) > 2.0) return out_of_range();
    from_f64(v, w, n);
    return FR_OK;
}

int fr_wide_add_double(uint64_t *w, uint32_t n, double delta) {
    const int rc = check_words(w, n);
    if (rc != FR_OK) return rc;
    if (!std::isfinite(delta)) return fr::fail(FR_ERR_INVALID_ARGUMENT, "fr_wide_add_double: delta is not finite");
    if (!within_two(w, n) || std::fabs(delta) > 4.0) return out_of_range();
    uint64_t d[kMaxWords];
    from_f64(delta, d, n);
    add_to(d, w, n);
    if (!within_two(d, n)) return out_of_range(); /* w is left as it was */
    memcpy(w, d, n * sizeof(uint64_t));
    return FR_OK;
}

int fr_wide_to_double(const uint64_t *w, uint32_t n, double *hi, double *lo) {
    const int rc = check_words(w, n);
    if (rc != FR_OK) return rc;
    if (!hi) return fr::fail(FR_ERR_INVALID_ARGUMENT, "fr_wide_to_double: hi is NULL");
    if (!within_two(w, n)) return out_of_range();
    const double h = to_f64(w, n);
    *hi = h;
    if (lo) { /* h is a multiple of 2^-F within the range: the rest is exact */
        uint64_t hw[kMaxWords], rest[kMaxWords];
        from_f64(h, hw, n);
        memcpy(rest, w, n * sizeof(uint64_t));
        sub_from(rest, hw, n);
        *lo = to_f64(rest, n);
    }
    return FR_OK;
}

int fr_wide_from_decimal(const char *text, uint64_t *w, uint32_t n) {
    const int rc = check_words(w, n);
    if (rc != FR_OK) return rc;
    const char *bad = "fr_wide_from_decimal: expected [+-]digits[.digits][e[+-]digits]";
    if (!text) return fr::fail(FR_ERR_INVALID_ARGUMENT, "fr_wide_from_decimal: text is NULL");
    if (strlen(text) > kMaxDecimalLength) return fr::fail(FR_ERR_INVALID_ARGUMENT, "fr_wide_from_decimal: the string is too long");
    const char *s = text;
    bool neg = false;
    if (*s == '+' || *s == '-') neg = *s++ == '-';
    Big mag; /* the digits as an integer; the value is mag 10^exp10 */
    size_t digits = 0, frac = 0;
    bool nonzero = false;
    size_t significant = 0; /* digits from the first non-zero one on */
    for (bool point = false;; s++) {
        if (*s == '.' && !point) {
            point = true;
            continue;
        }
        if (*s < '0' || *s > '9') break;
        big_mul_add(mag, 10, (uint64_t)(*s - '0'));
        digits++;
        frac += point ? 1 : 0;
        nonzero = nonzero || *s != '0';
        significant += nonzero ? 1 : 0;
    }
    if (digits == 0) return fr::fail(FR_ERR_INVALID_ARGUMENT, bad);
    long exp10 = 0;
    if (*s == 'e' || *s == 'E') {
        s++;
        bool eneg = false;
        if (*s == '+' || *s == '-') eneg = *s++ == '-';
        size_t ed = 0;
        for (; *s >= '0' && *s <= '9'; s++, ed++) exp10 = exp10 * 10 + (*s - '0');
        if (ed == 0 || ed > 4) return fr::fail(FR_ERR_INVALID_ARGUMENT, bad);
        if (eneg) exp10 = -exp10;
    }
    if (*s != '\0') return fr::fail(FR_ERR_INVALID_ARGUMENT, bad);
    exp10 -= (long)frac;
    if (nonzero && (long)significant + exp10 > 1) return out_of_range(); /* 10 or more */
    if (!nonzero) exp10 = 0;
    for (; exp10 > 0; exp10--) big_mul_add(mag, 10, 0);
    /* floor(mag 2^F / 10^k): floor divisions by positive integers compose */
    const uint32_t F = 64 * n - 8;
    Big num(F / 64, 0);
    for (uint64_t x : mag) num.push_back(x);
    if (!mag.empty()) big_mul_add(num, 1ull << (F % 64), 0);
    bool rest = false;
    long k = -exp10;
    for (; k >= 19; k -= 19) rest = big_div(num, 10000000000000000000ull) || rest;
    if (k > 0) {
        uint64_t d = 1;
        for (; k > 0; k--) d *= 10;
        rest = big_div(num, d) || rest;
    }
    if (neg && rest) { /* floor(-x) = -ceil(x) */
        Big one(num.size() + 1, 0);
        uint64_t carry = 1;
        for (size_t i = 0; i < one.size(); i++) {
            const uint64_t x = i < num.size() ? num[i] : 0;
            one[i] = x + carry;
            carry = (carry && one[i] == 0) ? 1 : 0;
        }
        while (!one.empty() && one.back() == 0) one.pop_back();
        num.swap(one);
    }
    if (num.size() > n) return out_of_range();
    uint64_t r[kMaxWords] = {};
    for (size_t i = 0; i < num.size(); i++) r[i] = num[i];
    if (negative(r, n)) return out_of_range(); /* a magnitude of 128 or more */
    if (neg) negate(r, n);
    if (!within_two(r, n)) return out_of_range();
    memcpy(w, r, n * sizeof(uint64_t));
    return FR_OK;
}

int fr_debug_reference_orbit_wide(const fr_config *cfg, const fr_wide_centre *centre, int which, double *out, size_t cap,
                                  uint32_t *len) {
    using namespace fr;
    const int rc = check_pt_wide(cfg, centre);
    if (rc != FR_OK) return rc;
    if (cfg->algo != 0 && cfg->algo != 2) return fail(FR_ERR_INVALID_ARGUMENT, "FR_PRECISION_PT: orbits exist for Mandelbrot and Julia");
    if (which != 0 && !(which == 1 && cfg->algo == 2))
        return fail(FR_ERR_INVALID_ARGUMENT, "which must be 0 (R or V) or, for Julia, 1 (K)");
    if (!len) return fail(FR_ERR_INVALID_ARGUMENT, "len is NULL");
    if (cap && !out) return fail(FR_ERR_INVALID_ARGUMENT, "out is NULL");
    std::vector<double> v;
    bool ended = false;
    WideTail tail;
    wide_reference_orbit(cfg, centre, which, v, ended, tail);
    *len = (uint32_t)(v.size() / 2);
    const size_t m = std::min(cap, v.size() / 2);
    if (m) memcpy(out, v.data(), m * 2 * sizeof(double));
    return FR_OK;
}
