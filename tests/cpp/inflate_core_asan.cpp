// The deflate decoder core (ukbb_cardiac_amd/csrc/inflate_core.h) compiled for the host, run over the corpus that
// tests/test_device_inflate.py writes, under -fsanitize=address,undefined.  Every stream is copied into a heap block of exactly
// src_len bytes and decoded into one of exactly dst_cap bytes: a byte read or written outside either is an AddressSanitizer error.
// File: uint32 count, then per case uint64 src_len, uint64 dst_cap, int64 expected result, the stream, and (result >= 0) the output.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "inflate_core.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (!rd(f, &count, 4)) return 2;
    for (uint32_t i = 0; i < count; ++i) {
        uint64_t src_len, cap; int64_t want;
        if (!rd(f, &src_len, 8) || !rd(f, &cap, 8) || !rd(f, &want, 8)) { fprintf(stderr, "case %u: short file\n", i); return 2; }
        std::vector<uint8_t> expect(want > 0 ? (size_t)want : 0), stream;
        for (int shift = 0; shift < 4; ++shift) {              // every alignment of the stream's first byte
            uint8_t *block = static_cast<uint8_t *>(malloc(src_len + shift ? src_len + shift : 1));
            uint8_t *src = block + shift;                      // the stream ends where the heap block ends
            if (shift == 0) {
                if (!rd(f, src, src_len) || !rd(f, expect.data(), expect.size())) { fprintf(stderr, "case %u: short file\n", i); return 2; }
                stream.assign(src, src + src_len);
            } else if (src_len) memcpy(src, stream.data(), src_len);
            uint8_t *dst = static_cast<uint8_t *>(malloc(cap ? cap : 1));
            ukbb_inflate::Work w;
            ukbb_inflate::HostIo io(src, dst);
            const int64_t got = ukbb_inflate::inflate_core(io, w, src_len, cap);
            if (got != want || (want > 0 && memcmp(dst, expect.data(), (size_t)want))) {
                fprintf(stderr, "case %u shift %d: got %lld, expected %lld%s\n", i, shift, (long long)got, (long long)want, got == want ? " (bytes differ)" : "");
                return 1;
            }
            free(dst);
            free(block);
        }
    }
    fclose(f);
    printf("inflate_core ok: %u cases\n", count);
    return 0;
}
