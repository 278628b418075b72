// Host check of csrc/quic.h (tests/test_quic_native.py): the functions quic_kernel.hip runs, compiled with g++, over the
// cases of the text file given as argv[1], written by the plain-Python reference (tests/quic_ref.py).  One case per line:
//   D <expected> <truncated> <pn_len> <want>                     quic_decode_pn (decimal)
//   P <pn_offset> <pn_len> <mask: 10 hex> <header hex> <want hex>  quic_protect_header, in place
//   U <pn_offset> <masked 0|1> <mask: 10 hex> <header hex> <want hex> <want pn_len> <want truncated>  quic_load_header +
//                                                                   quic_unprotect_header
// The header buffers are pn_offset + 4 bytes and a guard byte: whatever lies past the packet-number field must stay.
// Prints "ok <n>" or the first mismatch.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#define GF128_FN static inline
#include "quic.h"
using namespace ptls_hip;

static std::vector<uint8_t> unhex(const char *s)
{
    std::vector<uint8_t> v;
    for (size_t i = 0; s[i] != 0 && s[i + 1] != 0; i += 2) {
        unsigned b = 0;
        sscanf(s + i, "%2x", &b);
        v.push_back((uint8_t)b);
    }
    return v;
}

static void mask_words(const std::vector<uint8_t> &m, uint32_t &m0, uint32_t &m1)
{
    m0 = (uint32_t)m[0] | (uint32_t)m[1] << 8 | (uint32_t)m[2] << 16 | (uint32_t)m[3] << 24;
    m1 = (uint32_t)m[4] | 0xa5c3e100u; /* bytes 5..7 of the block are not the mask's: they must not matter */
}

int main(int argc, char **argv)
{
    if (argc < 2)
        return 2;
    FILE *f = fopen(argv[1], "r");
    if (f == nullptr)
        return 2;
    static char line[4096], a[1024], b[1024], c[1024];
    size_t n = 0;
    while (fgets(line, sizeof(line), f) != nullptr) {
        ++n;
        if (line[0] == 'D') {
            uint64_t expected, truncated, want;
            unsigned pn_len;
            if (sscanf(line + 1, "%" SCNu64 " %" SCNu64 " %u %" SCNu64, &expected, &truncated, &pn_len, &want) != 4)
                return printf("line %zu: bad case\n", n), 1;
            const uint64_t got = quic_decode_pn(expected, truncated, pn_len);
            if (got != want)
                return printf("line %zu: decode_pn(%" PRIu64 ", %" PRIu64 ", %u) = %" PRIu64 ", want %" PRIu64 "\n", n, expected,
                              truncated, pn_len, got, want),
                       1;
        } else if (line[0] == 'P') {
            unsigned pn_offset, pn_len;
            if (sscanf(line + 1, "%u %u %1023s %1023s %1023s", &pn_offset, &pn_len, a, b, c) != 5)
                return printf("line %zu: bad case\n", n), 1;
            std::vector<uint8_t> m = unhex(a), h = unhex(b), want = unhex(c);
            uint32_t m0, m1;
            mask_words(m, m0, m1);
            quic_protect_header(h.data(), pn_offset, pn_len, m0, m1);
            if (h != want)
                return printf("line %zu: protect_header mismatch\n", n), 1;
        } else if (line[0] == 'U') {
            unsigned pn_offset, masked, want_len;
            uint64_t want_trunc;
            if (sscanf(line + 1, "%u %u %1023s %1023s %1023s %u %" SCNu64, &pn_offset, &masked, a, b, c, &want_len, &want_trunc) != 7)
                return printf("line %zu: bad case\n", n), 1;
            std::vector<uint8_t> m = unhex(a), h = unhex(b), want = unhex(c);
            uint32_t m0, m1;
            mask_words(m, m0, m1);
            uint64_t trunc = ~(uint64_t)0;
            const uint32_t len = quic_unprotect_header(h.data(), pn_offset, quic_load_header(h.data(), pn_offset), masked != 0, m0, m1, &trunc);
            if (h != want || len != want_len || trunc != want_trunc)
                return printf("line %zu: unprotect_header: pn_len %u (want %u), truncated %" PRIu64 " (want %" PRIu64 ")%s\n", n,
                              len, want_len, trunc, want_trunc, h != want ? ", header bytes differ" : ""),
                       1;
        } else {
            return printf("line %zu: unknown case\n", n), 1;
        }
    }
    fclose(f);
    printf("ok %zu\n", n);
    return 0;
}
