// Host check of csrc/quic_keys.h (tests/test_quic_keys_native.py): the functions quic_keys.hip runs, compiled with g++, over
// the cases of the text file given as argv[1], whose expected values come from Python's hmac / hashlib.  One case per line
// ("-" stands for an empty byte string):
//   S <256|384> <key_size> <v2 0|1> <secret hex> <key> <iv> <hp> <next secret> <next key> <next iv>
//         hk_quic_keys_from_secret without the key update (key, iv, hp) and with it (next secret, its key and iv)
//   I <v2 0|1> <salt hex> <dcid hex> <server 0|1> <key> <iv> <hp>
//         hk_salt_pads + hk_quic_initial_keys
// Every output buffer is longer than what the call may write and starts as 0xA5: the bytes behind an output must stay.
// Prints "ok <n>" or the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#define GF128_FN static inline
#include "quic_keys.h"
using namespace ptls_hip;

typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const char *s)
{
    Bytes v;
    if (s[0] == '-')
        return v;
    for (size_t i = 0; s[i] != 0 && s[i + 1] != 0; i += 2) {
        unsigned b = 0;
        sscanf(s + i, "%2x", &b);
        v.push_back((uint8_t)b);
    }
    return v;
}

constexpr size_t CAP = 64;
constexpr uint8_t FILL = 0xA5;

/* buf[0 .. want.size()) == want and the rest of buf is untouched */
static bool same(const uint8_t (&buf)[CAP], const Bytes &want)
{
    if (std::memcmp(buf, want.data(), want.size()) != 0)
        return false;
    for (size_t i = want.size(); i < CAP; ++i)
        if (buf[i] != FILL)
            return false;
    return true;
}

template <class H>
static bool secret_case(const Bytes &secret, int update, int v2, uint32_t key_size, const Bytes &key, const Bytes &iv, const Bytes *hp,
                        const Bytes *next)
{
    uint8_t k[CAP], i[CAP], h[CAP], n[CAP];
    std::memset(k, FILL, CAP), std::memset(i, FILL, CAP), std::memset(h, FILL, CAP), std::memset(n, FILL, CAP);
    hk_quic_keys_from_secret<H>(secret.data(), update, v2, key_size, next != nullptr ? n : nullptr, k, i, hp != nullptr ? h : nullptr);
    return same(k, key) && same(i, iv) && same(h, hp != nullptr ? *hp : Bytes()) && same(n, next != nullptr ? *next : Bytes());
}

int main(int argc, char **argv)
{
    if (argc < 2)
        return 2;
    FILE *f = fopen(argv[1], "r");
    if (f == nullptr)
        return 2;
    static char line[4096], a[8][256];
    size_t n = 0;
    while (fgets(line, sizeof(line), f) != nullptr) {
        ++n;
        if (line[0] == 'S') {
            unsigned hash, key_size, v2;
            if (sscanf(line + 1, "%u %u %u %255s %255s %255s %255s %255s %255s %255s", &hash, &key_size, &v2, a[0], a[1], a[2], a[3], a[4],
                       a[5], a[6]) != 10)
                return printf("line %zu: bad case\n", n), 1;
            const Bytes secret = unhex(a[0]), key = unhex(a[1]), iv = unhex(a[2]), hp = unhex(a[3]), next = unhex(a[4]),
                        nkey = unhex(a[5]), niv = unhex(a[6]);
            if (secret.size() != hash / 8 || key.size() != key_size || hp.size() != key_size || iv.size() != 12 ||
                next.size() != secret.size() || nkey.size() != key_size || niv.size() != 12)
                return printf("line %zu: bad lengths\n", n), 1;
            const bool ok = hash == 256 ? secret_case<HkSha256>(secret, 0, (int)v2, key_size, key, iv, &hp, nullptr) &&
                                              secret_case<HkSha256>(secret, 1, (int)v2, key_size, nkey, niv, nullptr, &next)
                                        : secret_case<HkSha384>(secret, 0, (int)v2, key_size, key, iv, &hp, nullptr) &&
                                              secret_case<HkSha384>(secret, 1, (int)v2, key_size, nkey, niv, nullptr, &next);
            if (!ok)
                return printf("line %zu: keys of a secret differ (SHA-%u, key_size %u, v2 %u)\n", n, hash, key_size, v2), 1;
        } else if (line[0] == 'I') {
            unsigned v2, server;
            if (sscanf(line + 1, "%u %255s %255s %u %255s %255s %255s", &v2, a[0], a[1], &server, a[2], a[3], a[4]) != 7)
                return printf("line %zu: bad case\n", n), 1;
            const Bytes salt = unhex(a[0]), id = unhex(a[1]), key = unhex(a[2]), iv = unhex(a[3]), hp = unhex(a[4]);
            if (salt.empty() || salt.size() > HK_SALT_MAX || id.size() > HK_DCID_STRIDE || key.size() != 16 || iv.size() != 12 ||
                hp.size() != 16)
                return printf("line %zu: bad lengths\n", n), 1;
            uint8_t dcid[HK_DCID_STRIDE]; /* the entry of the 20-byte stride: the ID, then bytes that must not matter */
            std::memset(dcid, 0xEE, sizeof(dcid));
            std::memcpy(dcid, id.data(), id.size());
            HkPads<HkSha256> pads;
            hk_salt_pads(pads, salt.data(), salt.size());
            uint8_t k[CAP], i[CAP], h[CAP];
            std::memset(k, FILL, CAP), std::memset(i, FILL, CAP), std::memset(h, FILL, CAP);
            hk_quic_initial_keys(pads, dcid, (uint32_t)id.size(), (int)server, (int)v2, k, i, h);
            if (!same(k, key) || !same(i, iv) || !same(h, hp))
                return printf("line %zu: Initial keys differ (dcid %zu bytes, salt %zu bytes, server %u, v2 %u)\n", n, id.size(),
                              salt.size(), server, v2),
                       1;
        } else {
            return printf("line %zu: unknown case\n", n), 1;
        }
    }
    fclose(f);
    printf("ok %zu\n", n);
    return 0;
}
