// Host check of csrc/quic_parse.h (tests/test_quic_parse_native.py): the walk quic_parse_kernel.hip runs and the map
// functions quic_parse.cpp and the kernel share, compiled with g++ (and a second time with -fsanitize=address,undefined),
// over the cases of the text file given as argv[1], written by the plain-Python reference (tests/quic_parse_ref.py).  One
// case per line:
//   W <short_cid_len> <max_per_dgram> <require_fixed_bit> <datagram hex or -> <count> { <pos> <status> <type> <version>
//     <dcid_off> <dcid_len> <scid_off> <scid_len> <token_off> <token_len> <pn_offset> <pkt_len> <more> } x count
//   M new <capacity>          a fresh map: the table has the next power of two >= 2 * capacity entries
//   M set <cid hex or -> <conn>
//   M del <cid hex or ->
//   M get <cid hex or -> <want conn>      (4294967295 = no connection)
//   M size <want>
// Every datagram and every connection ID sits in a heap allocation of exactly its size, so that under AddressSanitizer a
// read of one byte past its end stops the run.  Prints "ok <n>" or the first mismatch.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#define GF128_FN static inline
#include "quic_parse.h"
using namespace ptls_hip;

// an allocation of exactly the bytes of `hex` ("-" = none: a 1-byte allocation nothing may read, *len = 0)
static uint8_t *exact(const std::string &hex, size_t *len)
{
    const size_t n = hex == "-" ? 0 : hex.size() / 2;
    uint8_t *p = static_cast<uint8_t *>(malloc(n != 0 ? n : 1));
    for (size_t i = 0; i < n; ++i)
        p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    *len = n;
    return n != 0 ? p : p + 1; /* the empty one: one past its allocation */
}

static void release(uint8_t *p, size_t len)
{
    free(len != 0 ? p : p - 1);
}

int main(int argc, char **argv)
{
    if (argc < 2)
        return 2;
    std::ifstream f(argv[1]);
    if (!f)
        return 2;
    std::string line;
    std::vector<QuicCidEntry> table;
    size_t count = 0, n = 0;
    const auto untouched = [](uint32_t) {};
    while (std::getline(f, line)) {
        ++n;
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "W") {
            uint32_t scl, max, fixed, want_count;
            std::string hex;
            in >> scl >> max >> fixed >> hex >> want_count;
            std::vector<uint64_t> want((size_t)want_count * 13);
            for (uint64_t &v : want)
                in >> v;
            if (!in) {
                printf("line %zu: malformed\n", n);
                return 1;
            }
            size_t len;
            uint8_t *d = exact(hex, &len);
            std::vector<uint64_t> got;
            const uint32_t k = quic_walk_datagram(d, (uint32_t)len, scl, max, fixed, [&got](uint32_t, uint32_t pos, const QuicWalk &w, bool more) {
                const uint64_t e[13] = {pos, w.status, w.type, w.version, w.dcid_off, w.dcid_len, w.scid_off, w.scid_len, w.token_off,
                                        w.token_len, w.pn_offset, w.pkt_len, more ? 1u : 0u};
                got.insert(got.end(), e, e + 13);
            });
            release(d, len);
            if (k != want_count || got != want) {
                printf("line %zu: walk mismatch: %u entries, want %u; got", n, k, want_count);
                for (uint64_t v : got)
                    printf(" %" PRIu64, v);
                printf("\n");
                return 1;
            }
        } else if (kind == "M") {
            std::string op, hex;
            in >> op;
            if (op == "new") {
                size_t capacity, size = 2;
                in >> capacity;
                while (size < 2 * capacity)
                    size <<= 1;
                table.assign(size, QuicCidEntry{});
                count = 0;
                continue;
            }
            if (op == "size") {
                size_t want;
                in >> want;
                if (want != count) {
                    printf("line %zu: size %zu, want %zu\n", n, count, want);
                    return 1;
                }
                continue;
            }
            in >> hex;
            size_t len;
            uint8_t *cid = exact(hex, &len);
            const uint32_t size = (uint32_t)table.size();
            bool ok = true;
            if (op == "set") {
                uint32_t conn;
                in >> conn;
                count += quic_cid_set(table.data(), size, cid, (uint32_t)len, conn, untouched) ? 1 : 0;
            } else if (op == "del") {
                count -= quic_cid_remove(table.data(), size, cid, (uint32_t)len, untouched) ? 1 : 0;
            } else if (op == "get") {
                uint32_t want;
                in >> want;
                const uint32_t got = quic_cid_lookup(table.data(), size, cid, (uint32_t)len);
                if (got != want) {
                    printf("line %zu: lookup gives %u, want %u\n", n, got, want);
                    ok = false;
                }
            } else {
                ok = false;
            }
            release(cid, len);
            if (!ok || !in)
                return 1;
        } else {
            printf("line %zu: unknown case\n", n);
            return 1;
        }
    }
    printf("ok %zu\n", n);
    return 0;
}
