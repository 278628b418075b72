/*
 * quic_scratch.h -- what the QUIC device objects share on the host (quic_scratch.cpp; part of host.h): the scan levels, the
 * owner of an object's device arrays and timing events, the plan sort, the keyset refusals.  The types have default
 * visibility like host.h's other objects (the ABI's object structs hold them); every function is hidden.
 */
#pragma once
#include <initializer_list>
#define QS_HIDDEN __attribute__((visibility("hidden")))

/* the levels of an exclusive scan over n counts (launch_quic_parse_scan), laid out in one allocation of `words` uint32 */
struct ScanLevels {
    uint32_t *l0, *l1, *l2, *total; /* the counts, the span sums (has1), their span sums (has2), the grand total */
    size_t n, n1, n2, words;
    bool has1, has2;
    ScanRef ref() const { return ScanRef{l0, has1 ? l1 : nullptr, has2 ? l2 : nullptr}; } /* what a kernel behind the scans reads */
};

/* the timing events of one owner (`count` of them, at most MAX), each created with its first mark; between() is 0 unless
 * both were marked.  No heap memory: the parse call builds one per call */
struct TimingEvents {
    static constexpr int MAX = 12;
    hipEvent_t ev[MAX] = {};
    const int count;
    explicit TimingEvents(int n) : count(n) {}
    ~TimingEvents() { destroy(); }
    QS_HIDDEN void destroy();
    QS_HIDDEN void mark(bool on, int k, hipStream_t s); /* on: the caller's thread-local timing switch */
    QS_HIDDEN float between(int a, int b) const;
    /* on, and event k was marked: waits for it (a diagnostic: the caller then reads between()) */
    QS_HIDDEN bool reached(bool on, int k) const;
};

/* one array of a group that grows together: its place in the object, its size at the new capacity, and the byte it is
 * filled with after growth (the value the kernels leave behind between calls), or no fill */
struct GrownArray {
    void **p;
    size_t bytes;
    int fill;
    template <class T>
    GrownArray(T **q, size_t b, int f = -1) : p(reinterpret_cast<void **>(q)), bytes(b), fill(f) {}
};

/* Every device array of a QUIC object comes from here, so release() needs no list of them.  The guarantees: an array is
 * freed only after uses.wait() (the object's launches, which its calls note in `uses`); a grown array is filled before the
 * new capacity is stored; release() waits, frees, destroys the timing events and synchronises eng->util, in that order. */
struct DeviceScratch {
    ptls_hip_engine_t *eng;
    const char *prefix; /* of the out-of-memory message: "quic_rx", "quic_tx" */
    Uses uses;          /* the launches that read or write the arrays */
    TimingEvents ev;
    static constexpr size_t MAX_ARRAYS = 24; /* (the receive object has 20; one more than this is refused, not lost) */
    void *owned[MAX_ARRAYS] = {};
    size_t n_owned = 0;

    DeviceScratch(ptls_hip_engine_t *e, const char *msg_prefix, int events) : eng(e), prefix(msg_prefix), ev(events) {}

    /* *p stays when it is allocated already; else `bytes` rounded up to 16 (ptls_hip_device_copy can read any array back) */
    template <class T>
    QS_HIDDEN int ensure(T **p, size_t bytes) { return ensure_bytes(reinterpret_cast<void **>(p), bytes); }
    QS_HIDDEN int ensure_bytes(void **p, size_t bytes);
    QS_HIDDEN int ensure_all(std::initializer_list<GrownArray> arrays); /* ensure() of each (no fill) */
    /* need <= *cap: nothing.  Else the arrays that exist are freed behind uses.wait(), all are allocated anew and filled on
     * `s`, and *cap = need (0 while any of this has failed) */
    QS_HIDDEN int grow(size_t *cap, size_t need, hipStream_t s, std::initializer_list<GrownArray> arrays);
    QS_HIDDEN void release();
};

/* the plan of the wave-per-record AES kernel: a stable order by two radix digits of the 12-bit sort keys */
struct PlanSort {
    uint32_t *d_order = nullptr, *d_order_tmp = nullptr;
    uint32_t *d_hist = nullptr; /* the [digit][tile] counts of a radix pass and their scan */

    /* the three arrays for up to cap positions; with their allocation d_order and d_order_tmp are zeroed on `s`, so that
     * every word a later pass could ever read as a position is a valid one */
    QS_HIDDEN int ensure(DeviceScratch &sc, size_t cap, hipStream_t s);
    /* d_order = the positions 0 .. m - 1 in plan order (quic_rx_kernel.hip's passes); 0 or the failed launch's hipError_t */
    QS_HIDDEN int sort(const uint32_t *d_keys, uint32_t m, int ncu, void *stream);
};

#pragma GCC visibility push(hidden)
ScanLevels scan_levels(uint32_t *base, size_t n); /* base == nullptr: for `words` alone */
int launch_scan_levels(const ScanLevels &L, int ncu, void *stream);
unsigned quic_scan_grid(size_t items, int ncu);
/* what a call of `object` ("receive object", "send object") refuses of its two keysets: another engine's, a header-protection
 * keyset of another algorithm or key size, and, with stride != 0, three key banks of that stride that do not fit ks */
int quic_keysets_check(const char *who, const char *object, const ptls_hip_engine_t *eng, const ptls_hip_keyset_t *ks,
                       const ptls_hip_keyset_t *hp_ks, size_t stride);
/* EINVAL "the <a_name> overlaps the <b_name>" when two non-empty byte ranges share a byte */
int quic_overlap_check(const char *who, const char *a_name, const void *a, size_t a_len, const char *b_name, const void *b,
                       size_t b_len);
#pragma GCC visibility pop
