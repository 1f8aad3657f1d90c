// Wavefront OBJ reader and writer on memory buffers -- plain C++17, no HIP: a host compiler builds this header alone (tests/host/obj_io_main.cpp).
//
// The reader restates etch_amd.inference_demo.load_obj line by line:
//   * a line ends at "\n", "\r\n" or a lone "\r" (Python's universal newlines); the last line needs no terminator;
//   * only lines whose first two bytes are "v " or "f " count (vn, vt, comments, blank and indented lines, "v<TAB>" are skipped);
//   * tokens are split on runs of the ASCII bytes str.split() treats as whitespace (9-13, 28-32);
//   * "v": the first three coordinates (float()), further tokens ignored; fewer than three is an error;
//   * "f": each token is the integer in front of its first '/', minus 1; a polygon is fanned (i0, ik, ik+1); fewer than three tokens yield
//     nothing (they are still parsed, as int() would).
// Unlike load_obj every stored index is checked against [0, nv): 0, negative (relative) and too large indices are errors.  nv is known from the
// count pass, so the check runs on the line itself and forward references stay legal.
// Numbers: std::from_chars (correctly rounded, no locale) where the library has it for double, else strtod_l in the "C" locale.  As float() and
// int() do: one leading '+' or '-', "inf" / "infinity" / "nan" in any case, '_' between two digits; no hex floats, no "nan(...)", nothing left
// over.  Not as they do: digits outside ASCII are rejected.  A magnitude past the double range becomes +-inf, below it 0 or a denormal.
//
// The writer restates Mesh.export: "v %.8f %.8f %.8f\n" per vertex, then "f %d %d %d\n" per face with 1-based indices.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <version>
#if defined(__cpp_lib_to_chars) && __cpp_lib_to_chars >= 201611L
#include <charconv>
#define ETCH_OBJ_HAVE_CHARCONV 1
#else
#define ETCH_OBJ_HAVE_CHARCONV 0
#endif
#include <locale.h>

namespace etch_obj {

enum : int {
    OK = 0,
    EINVAL_ = -1,      // a NULL pointer or a negative size
    EVERTEX = -3,      // a "v" line with fewer than three coordinates or a token float() rejects
    EFACE = -4,        // an "f" token int() rejects, or an integer outside int64
    EINDEX = -5,       // a face index outside [1, nv] in the file
    ECOUNT = -6,       // the buffer holds more vertices or faces than the arrays were sized for (counts of another buffer)
    ESPACE = -7,       // format: `cap` bytes do not hold the text; *written = the bytes it needs
};

inline bool is_space(unsigned char c) { return (c >= 9 && c <= 13) || (c >= 28 && c <= 32); }
inline bool is_digit(char c) { return c >= '0' && c <= '9'; }

// One line [p, e) without its terminator; *next = the first byte of the following line.
inline const char* line_end(const char* p, const char* end, const char** next) {
    const char* e = p;
    while (e < end && *e != '\n' && *e != '\r') ++e;
    *next = e < end ? ((*e == '\r' && e + 1 < end && e[1] == '\n') ? e + 2 : e + 1) : end;
    return e;
}

// The next token of [*p, e); false at the end of the line.
inline bool next_token(const char** p, const char* e, const char** tb, const char** te) {
    const char* q = *p;
    while (q < e && is_space((unsigned char)*q)) ++q;
    if (q == e) return false;
    *tb = q;
    while (q < e && !is_space((unsigned char)*q)) ++q;
    *te = q;
    *p = q;
    return true;
}

constexpr size_t TOKEN_MAX = 512;      // a number token with '_' or past the double range is copied; longer ones are rejected

// Python's rule for '_' in a numeric literal: only between two digits.  Copies [b, e) without them; false if misplaced or too long.
inline bool strip_underscores(const char* b, const char* e, char* buf, size_t* n) {
    size_t k = 0;
    for (const char* q = b; q < e; ++q) {
        if (*q == '_') {
            if (q == b || q + 1 == e || !is_digit(q[-1]) || !is_digit(q[1])) return false;
            continue;
        }
        if (k + 1 >= TOKEN_MAX) return false;
        buf[k++] = *q;
    }
    buf[k] = 0;
    *n = k;
    return true;
}

inline bool parse_double(const char* b, const char* e, double* out) {
    char buf[TOKEN_MAX];
    if (memchr(b, '_', (size_t)(e - b))) {
        size_t n;
        if (!strip_underscores(b, e, buf, &n)) return false;
        b = buf;
        e = buf + n;
    }
    if (b < e && *b == '+') {
        ++b;
        if (b < e && (*b == '+' || *b == '-')) return false;
    }
    if (b == e) return false;
    for (const char* q = b; q < e; ++q)
        if (*q == '(' || *q == 'x' || *q == 'X') return false;      // "nan(...)" and hex floats: float() takes neither
#if ETCH_OBJ_HAVE_CHARCONV
    const std::from_chars_result r = std::from_chars(b, e, *out);
    if (r.ptr != e) return false;
    if (r.ec == std::errc()) return true;
    if (r.ec != std::errc::result_out_of_range) return false;
    // past the double range from_chars gives no value; float() gives +-inf, 0 or a denormal, as strtod does
#else
    if (!(is_digit(*b) || *b == '-' || *b == '.' || *b == 'i' || *b == 'I' || *b == 'n' || *b == 'N')) return false;
#endif
    static const locale_t c_loc = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    if ((size_t)(e - b) + 1 > TOKEN_MAX) return false;
    const size_t n = (size_t)(e - b);
    memmove(buf, b, n);
    buf[n] = 0;
    char* endp = nullptr;
    *out = strtod_l(buf, &endp, c_loc);
    return endp == buf + n;
}

// int(token): false on a malformed token; *overflow when the digits are fine but the value is outside int64.
inline bool parse_int(const char* b, const char* e, int64_t* out, bool* overflow) {
    char buf[TOKEN_MAX];
    *overflow = false;
    if (memchr(b, '_', (size_t)(e - b))) {
        size_t n;
        if (!strip_underscores(b, e, buf, &n)) return false;
        b = buf;
        e = buf + n;
    }
    bool neg = false;
    if (b < e && (*b == '+' || *b == '-')) neg = *b++ == '-';
    if (b == e) return false;
    uint64_t v = 0;
    bool over = false;
    for (const char* q = b; q < e; ++q) {
        if (!is_digit(*q)) return false;
        const uint64_t d = (uint64_t)(*q - '0');
        if (v > (UINT64_MAX - d) / 10) over = true;
        v = v * 10 + d;
    }
    const uint64_t lim = neg ? (uint64_t)INT64_MAX + 1 : (uint64_t)INT64_MAX;
    if (over || v > lim) {
        *overflow = true;
        return true;
    }
    *out = neg ? (int64_t)(0 - v) : (int64_t)v;
    return true;
}

// Vertices and fanned triangles of the buffer.  Never fails on content: malformed lines are reported by parse().
inline int count(const char* data, int64_t len, int64_t* nv, int64_t* nf) {
    if (!nv || !nf || len < 0 || (!data && len > 0)) return EINVAL_;
    int64_t v = 0, f = 0;
    const char* p = data;
    const char* end = data + len;
    while (p < end) {
        const char* next;
        const char* e = line_end(p, end, &next);
        if (e - p >= 2 && p[1] == ' ') {
            if (p[0] == 'v') {
                ++v;
            } else if (p[0] == 'f') {
                const char* q = p + 1;
                const char *tb, *te;
                int64_t n = 0;
                while (next_token(&q, e, &tb, &te)) ++n;
                if (n >= 3) f += n - 2;
            }
        }
        p = next;
    }
    *nv = v;
    *nf = f;
    return OK;
}

// Fills v (nv,3) and f (nf,3) for the counts count() returned.  On an error *err_line = the 1-based line and the arrays hold rubbish.
inline int parse(const char* data, int64_t len, int64_t nv, int64_t nf, double* v, int64_t* f, int64_t* err_line) {
    if (!err_line || len < 0 || nv < 0 || nf < 0 || (!data && len > 0) || (!v && nv > 0) || (!f && nf > 0)) return EINVAL_;
    *err_line = 0;
    int64_t vi = 0, fi = 0, line = 0;
    const char* p = data;
    const char* end = data + len;
    while (p < end) {
        const char* next;
        const char* e = line_end(p, end, &next);
        ++line;
        if (e - p >= 2 && p[1] == ' ' && (p[0] == 'v' || p[0] == 'f')) {
            *err_line = line;
            const char* q = p + 1;
            const char *tb, *te;
            if (p[0] == 'v') {
                if (vi >= nv) return ECOUNT;
                int k = 0;
                for (; k < 3 && next_token(&q, e, &tb, &te); ++k)
                    if (!parse_double(tb, te, &v[vi * 3 + k])) return EVERTEX;
                if (k < 3) return EVERTEX;
                ++vi;
            } else {
                int64_t i0 = 0, prev = 0, n = 0;
                while (next_token(&q, e, &tb, &te)) {
                    const char* s = tb;
                    while (s < te && *s != '/') ++s;
                    int64_t idx = 0;
                    bool over = false;
                    if (!parse_int(tb, s, &idx, &over) || over) return EFACE;
                    ++n;
                    if (n == 1) {
                        i0 = idx;
                    } else if (n >= 3) {
                        // a stored triangle: every corner must name a vertex of the file
                        if (i0 < 1 || i0 > nv || prev < 1 || prev > nv || idx < 1 || idx > nv) return EINDEX;
                        if (fi >= nf) return ECOUNT;
                        f[fi * 3] = i0 - 1;
                        f[fi * 3 + 1] = prev - 1;
                        f[fi * 3 + 2] = idx - 1;
                        ++fi;
                    }
                    prev = idx;
                }
            }
        }
        p = next;
    }
    if (vi != nv || fi != nf) {
        *err_line = line;
        return ECOUNT;
    }
    *err_line = 0;
    return OK;
}

constexpr size_t NUMBER_MAX = 352;      // "%.8f" of the largest double: sign, 309 digits, '.', 8 digits

// "%.8f": correctly rounded, '.' whatever the locale; nan without a sign, as Python's % prints it.
inline size_t format_f8(double x, char* buf) {
    if (x != x) {
        memcpy(buf, "nan", 3);
        return 3;
    }
#if ETCH_OBJ_HAVE_CHARCONV
    return (size_t)(std::to_chars(buf, buf + NUMBER_MAX, x, std::chars_format::fixed, 8).ptr - buf);
#else
    const int n = snprintf(buf, NUMBER_MAX, "%.8f", x);
    for (int i = 0; i < n; ++i)
        if (buf[i] == ',') buf[i] = '.';
    return (size_t)n;
#endif
}

inline size_t format_i64(int64_t x, char* buf) {
    char tmp[24];
    size_t n = 0, k = 0;
    uint64_t u = x < 0 ? 0 - (uint64_t)x : (uint64_t)x;
    do {
        tmp[n++] = (char)('0' + u % 10);
        u /= 10;
    } while (u);
    if (x < 0) buf[k++] = '-';
    while (n) buf[k++] = tmp[--n];
    return k;
}

// Writes the text of Mesh(v (nv,3), f (nf,3)).export into out[0, cap).  *written = the bytes of the whole text; ESPACE (and nothing past
// cap touched) when that is more than cap: call again with that many.
inline int format(const double* v, int64_t nv, const int64_t* f, int64_t nf, char* out, int64_t cap, int64_t* written) {
    if (!written || nv < 0 || nf < 0 || cap < 0 || (!v && nv > 0) || (!f && nf > 0) || (!out && cap > 0)) return EINVAL_;
    char buf[3 * NUMBER_MAX + 8];
    int64_t pos = 0;
    for (int64_t i = 0; i < nv + nf; ++i) {
        size_t n = 0;
        buf[n++] = i < nv ? 'v' : 'f';
        for (int c = 0; c < 3; ++c) {
            buf[n++] = ' ';
            n += i < nv ? format_f8(v[i * 3 + c], buf + n) : format_i64((int64_t)((uint64_t)f[(i - nv) * 3 + c] + 1), buf + n);
        }
        buf[n++] = '\n';
        if (pos + (int64_t)n <= cap) memcpy(out + pos, buf, n);
        pos += (int64_t)n;
    }
    *written = pos;
    return pos <= cap ? OK : ESPACE;
}

}  // namespace etch_obj
