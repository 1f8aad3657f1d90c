// C ABI of the OBJ reader and writer (obj_io.h: host C++ only, no kernel in this translation unit).  The calls work on memory buffers and hold
// no state, so a Python thread pool runs several at once (ctypes releases the GIL for the call).
#include "etch_hip.h"
#include "obj_io.h"

static_assert(etch_obj::EVERTEX == ETCH_OBJ_EVERTEX && etch_obj::EFACE == ETCH_OBJ_EFACE && etch_obj::EINDEX == ETCH_OBJ_EINDEX &&
                  etch_obj::ECOUNT == ETCH_OBJ_ECOUNT && etch_obj::ESPACE == ETCH_OBJ_ESPACE,
              "obj_io.h and etch_hip.h disagree on the status codes");

extern "C" {

int etch_obj_count(const char* data, long long len, long long* nv, long long* nf) {
    int64_t v = 0, f = 0;
    if (!nv || !nf) return etch_obj::EINVAL_;
    const int r = etch_obj::count(data, (int64_t)len, &v, &f);
    *nv = v;
    *nf = f;
    return r;
}

int etch_obj_parse(const char* data, long long len, long long nv, long long nf, double* v, long long* f, long long* err_line) {
    static_assert(sizeof(long long) == sizeof(int64_t), "faces are int64");
    int64_t line = 0;
    if (!err_line) return etch_obj::EINVAL_;
    const int r = etch_obj::parse(data, (int64_t)len, (int64_t)nv, (int64_t)nf, v, (int64_t*)f, &line);
    *err_line = line;
    return r;
}

int etch_obj_format(const double* v, long long nv, const long long* f, long long nf, char* out, long long cap, long long* written) {
    int64_t w = 0;
    if (!written) return etch_obj::EINVAL_;
    const int r = etch_obj::format(v, (int64_t)nv, (const int64_t*)f, (int64_t)nf, out, (int64_t)cap, &w);
    *written = w;
    return r;
}

}  // extern "C"
