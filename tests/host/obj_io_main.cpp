// Stand-alone driver of etch_amd/csrc/obj_io.h for a sanitizer build (tests/test_ingest_host.py compiles it with -fsanitize=address,undefined).
//   obj_io_main GOOD.obj [OTHER.obj ...]
// Every file goes through count, parse and (when it parses) format and a second parse of the formatted text.  Each input is copied into a heap
// block of exactly its size, so one byte read past the text is an error the sanitizer reports.  The first file is also cut at every byte offset of
// its first 200 bytes.  One line per file on stdout: "<path> rc=<status> line=<error line> nv=<vertices> nf=<triangles>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "obj_io.h"

struct Result {
    int rc;
    int64_t line, nv, nf;
};

static Result run(const char* text, size_t len) {
    char* data = (char*)malloc(len ? len : 1);
    memcpy(data, text, len);
    Result r{0, 0, 0, 0};
    r.rc = etch_obj::count(data, (int64_t)len, &r.nv, &r.nf);
    if (r.rc == 0) {
        std::vector<double> v((size_t)r.nv * 3);
        std::vector<int64_t> f((size_t)r.nf * 3);
        r.rc = etch_obj::parse(data, (int64_t)len, r.nv, r.nf, v.data(), f.data(), &r.line);
        if (r.rc == 0) {
            int64_t need = 0, again = 0;
            char probe[8];
            const int e = etch_obj::format(v.data(), r.nv, f.data(), r.nf, probe, 8, &need);      // too small on purpose: reports the size
            if (e != 0 && e != etch_obj::ESPACE) r.rc = 100;
            char* out = (char*)malloc(need ? (size_t)need : 1);
            if (etch_obj::format(v.data(), r.nv, f.data(), r.nf, out, need, &again) != 0 || again != need) r.rc = 101;
            int64_t nv2 = 0, nf2 = 0, line2 = 0;
            if (etch_obj::count(out, need, &nv2, &nf2) != 0 || nv2 != r.nv || nf2 != r.nf) r.rc = 102;
            std::vector<double> v2((size_t)nv2 * 3);
            std::vector<int64_t> f2((size_t)nf2 * 3);
            if (r.rc == 0 && (etch_obj::parse(out, need, nv2, nf2, v2.data(), f2.data(), &line2) != 0 || f2 != f)) r.rc = 103;
            free(out);
        }
    }
    free(data);
    return r;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* fh = fopen(argv[a], "rb");
        if (!fh) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<char> text;
        char buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, fh)) > 0) text.insert(text.end(), buf, buf + n);
        fclose(fh);
        const Result r = run(text.data(), text.size());
        printf("%s rc=%d line=%lld nv=%lld nf=%lld\n", argv[a], r.rc, (long long)r.line, (long long)r.nv, (long long)r.nf);
        if (a == 1)
            for (size_t cut = 0; cut <= text.size() && cut <= 200; ++cut) {
                const Result t = run(text.data(), cut);
                if (t.rc >= 100) {
                    printf("truncation at %zu: rc=%d\n", cut, t.rc);
                    return 1;
                }
            }
    }
    printf("done\n");
    return 0;
}
