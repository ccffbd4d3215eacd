// The parallel formulation of the label-volume gzip writer (ukbb_fcn_gzip_labels_parallel_host: label_gzip_core.h run step by step, as
// the device encoder runs it) and the serial writer, compiled for the host under -fsanitize=address,undefined and run over the corpus
// that tests/test_device_label_gzip.py writes: every datatype, both code sets, equal bytes.  Labels, prefix and output live in heap
// blocks of exactly n_voxels, prefix_len and out_cap bytes: a byte read or written outside any of them is an AddressSanitizer error.
// The two declines are run with exact-size blocks as well.  File: uint32 count, then per volume uint64 n_voxels, uint64 prefix_len,
// the prefix, the labels.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ukbb_fcn.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (!rd(f, &count, 4)) return 2;
    static const int datatypes[5] = {2, 4, 8, 16, 64};
    for (uint32_t i = 0; i < count; ++i) {
        uint64_t n, plen;
        if (!rd(f, &n, 8) || !rd(f, &plen, 8)) { fprintf(stderr, "volume %u: short file\n", i); return 2; }
        uint8_t *prefix = static_cast<uint8_t *>(malloc(plen ? plen : 1)), *labels = static_cast<uint8_t *>(malloc(n ? n : 1));
        if (!rd(f, prefix, plen) || !rd(f, labels, n)) { fprintf(stderr, "volume %u: short file\n", i); return 2; }
        uint64_t runs = 0;
        for (uint64_t k = 0; k < n; ++k) runs += k == 0 || labels[k] != labels[k - 1];
        for (int d = 0; d < 5; ++d)
            for (int mode = 0; mode < 2; ++mode) {
                const uint64_t bound = ukbb_fcn_gzip_labels_bound(n, datatypes[d], plen);
                uint8_t *ref = static_cast<uint8_t *>(malloc(bound));
                const int64_t want = ukbb_fcn_gzip_labels_mode(labels, n, datatypes[d], prefix, plen, ref, bound, mode);
                if (want < 0) { fprintf(stderr, "volume %u datatype %d mode %d: the serial writer returned %lld\n", i, datatypes[d], mode, (long long)want); return 1; }
                uint8_t *out = static_cast<uint8_t *>(malloc((size_t)want));                       // exactly the member
                const int64_t got = ukbb_fcn_gzip_labels_parallel_host(labels, n, datatypes[d], prefix, plen, mode, out, (uint64_t)want, runs);
                if (got != want || memcmp(out, ref, (size_t)want)) {
                    fprintf(stderr, "volume %u datatype %d mode %d: got %lld, expected %lld%s\n", i, datatypes[d], mode, (long long)got, (long long)want,
                            got == want ? " (bytes differ)" : "");
                    return 1;
                }
                free(out);
                out = static_cast<uint8_t *>(malloc((size_t)want - 1));                            // one byte short
                if (ukbb_fcn_gzip_labels_parallel_host(labels, n, datatypes[d], prefix, plen, mode, out, (uint64_t)want - 1, runs) != UKBB_LABELGZ_NO_ROOM) {
                    fprintf(stderr, "volume %u datatype %d mode %d: no decline with out_cap one byte short\n", i, datatypes[d], mode);
                    return 1;
                }
                if (runs > 1 && ukbb_fcn_gzip_labels_parallel_host(labels, n, datatypes[d], prefix, plen, mode, out, (uint64_t)want - 1, runs - 1) !=
                                    UKBB_LABELGZ_TOO_MANY_RUNS) {
                    fprintf(stderr, "volume %u datatype %d mode %d: no decline with one run too many\n", i, datatypes[d], mode);
                    return 1;
                }
                free(out);
                free(ref);
            }
        free(labels);
        free(prefix);
    }
    fclose(f);
    printf("label_gzip_core ok: %u volumes\n", count);
    return 0;
}
