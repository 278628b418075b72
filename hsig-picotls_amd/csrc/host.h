/*
 * host.h -- what the host-side units of libptls_hip.so share (not part of the C ABI; every declaration here has hidden
 * visibility, so the library exports only include/ptls_hip.h).
 *
 *   engine.cpp         errors, the AES T-table, engines (device memory pool, chunk queues), the start-up self-check
 *   keyset.cpp         keysets: AES key slots + GHASH basis, or ChaCha key slots; keys / IVs / TLS 1.3 secrets / QUIC
 *                      secrets and Initial keys (kernels: keyschedule.hip, quic_keys.hip; the QUIC arithmetic shared with
 *                      the CPU check: quic_keys.h)
 *   planner.cpp        the launch planner: lanes per record, chunks, grid
 *   batch.cpp          batches and the device-resident seal / open / header-protection calls; the one record launch of a
 *                      plan (launch_plan, run_plan), which the pipelines and the receive object share
 *   quic.cpp           QUIC packet protection batches: header protection on the device around the record calls, and the two
 *                      header steps every QUIC path launches through (quic_unprotect, quic_protect)
 *                      (kernels: quic_kernel.hip; the header arithmetic shared with the CPU check: quic.h)
 *   quic_scratch.cpp   what the QUIC device objects below share: the scan levels, the owner of an object's device arrays and
 *                      timing events (DeviceScratch), the plan sort, the keyset and overlap refusals (quic_scratch.h; the
 *                      device-side counterpart of the scan lookup: quic_scan.h)
 *   quic_parse.cpp     QUIC datagrams parsed on the device into the packet descriptors of quic.cpp, and the connection-ID map
 *                      (kernels: quic_parse_kernel.hip; the walk and the map arithmetic shared with the CPU check: quic_parse.h)
 *   quic_rx.cpp        the QUIC receive object: parsed entries kept on the device, selected, packed, planned and opened there
 *                      (kernels: quic_rx_kernel.hip; the select rule and the sums' terms shared with the CPU check: quic_rx.h),
 *                      and on it the key chosen by Key Phase bit and the commit of key updates (kernels:
 *                      quic_phase_kernel.hip; the rule shared with the CPU check: quic_phase.h), and the received packet
 *                      numbers tracked behind an open call (kernels: quic_track_kernel.hip; the rule: quic_track.h), and
 *                      the ACK frames and send requests written from them (kernels: quic_ack_kernel.hip; the rule: quic_ack.h)
 *   quic_tx.cpp        the QUIC send object: requests in device memory numbered, given headers and a key generation from a
 *                      per-connection state table on the device, compacted, planned and sealed there (kernels:
 *                      quic_tx_kernel.hip; the rule shared with the CPU check: quic_tx.h)
 *   tls13.cpp          the TLS 1.3 record layer over the batch (framing, parsing)
 *   slice_plan.cpp     the copy transport's planning: a slice's cut, descriptors, copies back, gaps, mask places, and for
 *                      QUIC packets the headers and plaintext tails staged with the gaps (no HIP call)
 *   pipeline.cpp       host-resident records and QUIC packets: the mapped and copy transports over one slice loop
 *                      (run_slices) and one slice launcher (launch_slice: it plans, uploads and calls batch.cpp's
 *                      launch_plan), for AES-GCM or ChaCha20-Poly1305 keysets (the latter: chacha_kernel.hip,
 *                      chacha_runs_kernel.hip; the copy transport's QUIC header return: quic_slice_kernel.hip)
 *   node.cpp           one batch over several devices, NUMA placement
 *   plugin_worker.cpp  the picotls plugin's runtime: the resident worker dispatch and pooled resources
 *   plugin.cpp         the picotls plugin objects (AEAD, CTR, ECB, fusion-style low-level API)
 */
#ifndef PTLS_HIP_HOST_H
#define PTLS_HIP_HOST_H

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "internal.h"

using namespace ptls_hip;

/* (the functions and variables below are hidden; the object types are plain structs without vtables) */
#pragma GCC visibility push(hidden)

/* ---- errors (engine.cpp) ---- */

/* the calling thread's last error message (ptls_hip_last_error) */
extern thread_local std::string g_err;
/* records a formatted message as the thread's last error and returns `code` */
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr, code)                                                                                                        \
    do {                                                                                                                           \
        hipError_t e_ = (expr);                                                                                                    \
        if (e_ != hipSuccess)                                                                                                      \
            return fail((code), "%s failed: %s", #expr, hipGetErrorString(e_));                                                  \
    } while (0)

#pragma GCC visibility pop

/* ---------------------------------------------------------------------------------------------- */
/* objects                                                                                         */
/* ---------------------------------------------------------------------------------------------- */

struct st_ptls_hip_engine_t {
    int device;
    int ncu;
    uint32_t *d_t0;
    uint32_t *d_queue;                /* QUEUE_SLOTS x {next chunk, workgroups done}: the batch kernel's chunk queues */
    std::atomic<uint32_t> queue_next; /* the slot the next batch launch takes */
    uint32_t queue_slots;             /* slots in the round robin: QUEUE_SLOTS (PTLS_HIP_QUEUE_SLOTS: fewer, for tests) */
    hipStream_t util;                 /* descriptor / keyset allocation, zeroing and release (dev_alloc / dev_free) */
    hipMemPool_t pool;                /* the engine's own device memory pool (dev_alloc), or nullptr: hipMalloc */
};

/* the streams launches on an object went to, each with an event recorded after its last such launch: freeing the object
 * (or re-planning a batch) waits for exactly that work */
struct Uses {
    std::mutex mu;
    std::vector<std::pair<hipStream_t, hipEvent_t>> v;

    void note(void *stream)
    {
        hipStream_t st = static_cast<hipStream_t>(stream);
        std::lock_guard<std::mutex> lk(mu);
        for (auto &u : v)
            if (u.first == st) {
                (void)hipEventRecord(u.second, st);
                return;
            }
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, st) == hipSuccess)
            v.emplace_back(st, ev);
        else /* no event: the wait falls back to the whole device */
            v.emplace_back(st, nullptr);
    }

    void wait()
    {
        std::lock_guard<std::mutex> lk(mu);
        bool device_wide = false;
        for (auto &u : v) {
            if (u.second == nullptr) {
                device_wide = true;
                continue;
            }
            (void)hipEventSynchronize(u.second);
        }
        if (device_wide)
            (void)hipDeviceSynchronize();
    }

    ~Uses()
    {
        for (auto &u : v)
            if (u.second != nullptr)
                (void)hipEventDestroy(u.second);
    }
};

struct st_ptls_hip_keyset_t {
    ptls_hip_engine_t *eng;
    size_t key_size, nslots;
    int algo = PTLS_HIP_ALGO_AESGCM; /* PTLS_HIP_ALGO_*: which of the two slot arrays below exists */
    KeySlot *d_slots;     /* AES-GCM: key schedule, IV, H powers */
    uint32_t *d_basis;    /* AES-GCM: the GHASH basis */
    ChaChaSlot *d_chacha = nullptr; /* ChaCha20-Poly1305: key + IV, 44 bytes per slot (no basis, no KeySlot) */
    std::vector<uint8_t> ivs; /* host mirror of every slot's static IV (do_get_iv) */
    int64_t pool_id = -1;     /* >= 0: a plugin context's slot from the plugin pool (pool_keyset), not its own allocation */
    Uses uses; /* launches that read this keyset: keyset_free waits for exactly that work */
};

/* after a launch on `stream` that reads ks */
inline void keyset_note_use(ptls_hip_keyset_t *ks, void *stream)
{
    if (ks != nullptr && ks->pool_id < 0)
        ks->uses.note(stream);
}

struct st_ptls_hip_batch_t {
    ptls_hip_engine_t *eng;
    size_t n;
    ptls_hip_record_t *d_recs;
    ptls_hip_record_t *d_recs_ord; /* descriptors in chunk order (the batch kernel's view) */
    std::vector<ptls_hip_record_t> h_recs;
    Chunk *d_chunks;
    uint32_t *d_order;
    uint32_t nchunks;
    int lanes;      /* in use */
    int wg;         /* threads per workgroup */
    int forced_wg;  /* 0 = plan_wg */
    bool all_aligned; /* every descriptor's in/out/aad offset is a multiple of 16 */
    int auto_lanes; /* chosen from the record lengths */
    bool forced;
    int chacha_lanes;      /* lanes per record of the ChaCha kernel, in use (1, 4, 16, 64) */
    int chacha_auto_lanes; /* chosen from the record lengths */
    uint32_t max_key; /* largest key slot any record names (checked against the keyset at seal/open) */
    unsigned max_wg;  /* 0, or a cap on the workgroups of a launch (planning then sizes chunks for that many) */
    uint64_t *d_clk;  /* diagnostic clock stamps of the next launches (ptls_hip_batch_set_clock), or nullptr */
    size_t clk_bytes;
    Uses uses;        /* launches that read the descriptors and the plan: re-planning and batch_free wait for them */
};

/* CUs a batch is planned and launched for: the device's, or fewer when the batch caps its grid */
inline unsigned batch_cus(const st_ptls_hip_batch_t *b)
{
    const unsigned ncu = (unsigned)b->eng->ncu;
    return b->max_wg != 0 && b->max_wg < ncu ? b->max_wg : ncu;
}

/* the grid of the one-thread-per-record kernels (TLS 1.3 headers / inner plaintext, stand-alone masks): 256 threads per
 * workgroup, at most four workgroups per CU */
inline unsigned record_grid(size_t n, int ncu)
{
    const size_t wgs = (n + 255) / 256, cap = (size_t)ncu * 4;
    return (unsigned)(wgs < cap ? wgs : cap);
}

/* the key material of an AES-GCM launch: the keyset's slots and basis, the engine's T-table, the header-protection slots */
inline void set_key_args(KernelArgs &a, const ptls_hip_engine_t *eng, const ptls_hip_keyset_t *ks, const ptls_hip_keyset_t *hp_ks)
{
    a.slots = ks->d_slots;
    a.basis = ks->d_basis;
    a.t0 = eng->d_t0;
    a.hp_slots = hp_ks != nullptr ? hp_ks->d_slots : nullptr;
    a.hp_nslots = hp_ks != nullptr ? (uint32_t)hp_ks->nslots : 0;
}

/* (pipeline.cpp, slice_plan.cpp) where slot_wait puts the unprotected header bytes of an opened packet: h_pkt + off and h_pkt + off + pn_offset */
struct HdrDst {
    uint64_t off;
    uint32_t pn_offset;
};

class DeviceGuard {
  public:
    explicit DeviceGuard(int dev)
    {
        (void)hipGetDevice(&prev_);
        if (prev_ != dev)
            (void)hipSetDevice(dev);
        dev_ = dev;
    }
    ~DeviceGuard()
    {
        if (prev_ != dev_)
            (void)hipSetDevice(prev_);
    }

  private:
    int prev_ = 0, dev_ = 0;
};

#include "quic_scratch.h" /* (quic_scratch.cpp: its types belong here, its functions are hidden as those below) */

#pragma GCC visibility push(hidden)

/* uint32 words of one key slot's GHASH basis (internal.h BASIS_VECS uint4) */
constexpr size_t BASIS_WORDS_PER_SLOT = (size_t)BASIS_VECS * 4;

/* ---- engine.cpp ---- */
/* stream-ordered device memory from the engine's own pool (hipMalloc / hipFree without one) */
hipError_t dev_alloc(ptls_hip_engine_t *e, void **p, size_t bytes);
void dev_free(ptls_hip_engine_t *e, void *p);
/* the chunk-queue words of one batch-kernel launch */
uint32_t *queue_slot(ptls_hip_engine_t *e);

/* ---- planner.cpp ---- */
int choose_lanes(const ptls_hip_record_t *recs, size_t n, unsigned ncu);
int choose_chacha_lanes(const ptls_hip_record_t *recs, size_t n, unsigned ncu);
/* the same rules over the sums the two functions above take (n != 0) */
int choose_lanes_from(double sum, size_t n, size_t runs, unsigned ncu);
int choose_chacha_lanes_from(double sum, size_t n, unsigned ncu);
unsigned plan_grid(size_t n, size_t nchunks, int lanes, unsigned ncu);
int plan_wg(const std::vector<Chunk> &ch, int lanes);
void build_chunks(const ptls_hip_record_t *recs, size_t n, int lanes, unsigned ncu, std::vector<Chunk> &ch,
                  std::vector<uint32_t> &order, bool &all_aligned);
bool identity_order(const std::vector<uint32_t> &order, size_t n);
/* every descriptor's in / out / aad offset is a multiple of 16: what build_chunks reports as all_aligned */
bool offsets_aligned(const ptls_hip_record_t *recs, size_t n);

/* ---- slice_plan.cpp: what the copy transport places where, per slice (arithmetic on descriptors, no HIP call) ---- */
/* what a pipeline slice runs: plain seal / open (AAD in its own buffer), or the TLS 1.3 record layer
 * (seal: the 5-byte headers are written into the output and read back as the AAD, like
 * ptls_hip_tls13_seal_batch; open: the AAD is the header in the received input, and the inner plaintext
 * is parsed after the open, like ptls_hip_tls13_open_batch), or QUIC packet protection (seal: the AAD is the header the
 * caller wrote into the packet, in the output; open: the header in the received packet, in the input; no TLS framing,
 * the header-protection kernels of quic_kernel.hip run around the record kernel instead) */
enum PipeMode { PIPE_SEAL, PIPE_OPEN, PIPE_TLS13_SEAL, PIPE_TLS13_OPEN, PIPE_QUIC_SEAL, PIPE_QUIC_OPEN };

/* what the mode means for the buffers: which side carries the tag, and the buffer the AAD lives in */
struct ModeInfo {
    bool open;
    bool aad_in_out, aad_in_in; /* the AAD is the header in the output (TLS 1.3 / QUIC seal) / in the input (... open) */
    uint32_t tag_in, tag_out;   /* tag bytes after a record's input / output */
    bool quic;                  /* QUIC packets: the header is the caller's (seal) or the packet's (open), not a TLS 1.3 one */
    ModeInfo(PipeMode m)
        : open(m == PIPE_OPEN || m == PIPE_TLS13_OPEN || m == PIPE_QUIC_OPEN), aad_in_out(m == PIPE_TLS13_SEAL || m == PIPE_QUIC_SEAL),
          aad_in_in(m == PIPE_TLS13_OPEN || m == PIPE_QUIC_OPEN), tag_in(open ? 16 : 0), tag_out(open ? 0 : 16),
          quic(m == PIPE_QUIC_SEAL || m == PIPE_QUIC_OPEN)
    {
    }
};

/* byte range [lo, hi) */
struct Span {
    uint64_t lo, hi;
};

constexpr size_t COPY_DIRECT_RUNS = 8;   /* at most this many runs per slice: one copy each, no gap is written */
constexpr uint64_t GAP_SPLIT = 64 << 10; /* a gap this long splits the copy instead of being filled */
/* masks per slice: the slot's d_mask holds slice_bytes / 4 */
constexpr size_t slot_max_masks(size_t slice_bytes)
{
    return slice_bytes / 64;
}

/* per call: the records are in output order (each record's output starts at or after the previous one's end, the usual
 * layout), so a slice's gaps hold no other slice's bytes; otherwise `uni`, the merged union of every record's output,
 * decides that */
struct CopyOrder {
    bool in_order;
    std::vector<Span> uni;
};
void plan_copy_order(const ptls_hip_record_t *recs, size_t n, const ModeInfo &m, CopyOrder &o);

/* per slice: records [i, j) and everything the host places for them */
struct SlicePlan {
    size_t j;
    Span in, out, aad;                    /* the bytes of the caller's buffers the slice stages (aad: {0, 0} if none) */
    uint64_t in_base, out_base, aad_base; /* what the slice-local offsets are relative to: the span starts, rounded down to 16 */
    std::vector<ptls_hip_record_t> recs;  /* slice-local descriptors */
    std::vector<ptls_hip_supp_t> supp;    /* ... and header-protection descriptors (empty without supp) */
    std::vector<Span> pieces;             /* the D2H copies of the output, in the caller's offsets */
    std::vector<GapPiece> gaps;           /* the gaps inside the pieces, filled in the staging before the kernels run ... */
    std::vector<Span> gap_src;            /* ... with these bytes of the caller's output */
    std::vector<uint64_t> mask_dst;       /* the caller's mask_off of the t-th mask the kernel writes (local mask_off 16 t) */
    std::vector<Span> runs;               /* scratch: the records' merged output runs */
};
/* the greedy cut from record i against the staging limits (slice_bytes of input and output, slice_bytes / 4 of AAD,
 * slot_max_masks masks, max_recs - 1 records), then the slice's plan; EINVAL for a record that does not fit a slice or a
 * header-protection sample outside the slice's output */
int plan_copy_slice(const ptls_hip_record_t *recs, const ptls_hip_supp_t *supp, size_t n, size_t i, const ModeInfo &m,
                    size_t slice_bytes, size_t max_recs, size_t hp_nslots, const CopyOrder &o, SlicePlan &pl);

/* QUIC packets through the pipelines (ptls_hip_pipeline_quic_seal / _open).  quic_records: the record and header-protection
 * descriptors of the packets as quic.cpp builds them per batch, in the caller's offsets (seal: supp[i] = sample at
 * pn_offset + 4, mask at 16 i; open: from pn_len = 1, the packet-number length sits under header protection, so the record
 * lengths are the plaintext AREAS pkt_len - pn_offset - 17, up to 3 bytes more than the kernel will write). */
void quic_records(const ptls_hip_quic_packet_t *pkts, size_t n, bool open, std::vector<ptls_hip_record_t> &recs,
                  std::vector<ptls_hip_supp_t> &supp);
/* the per-packet refusals of ptls_hip_quic_batch_new; nullptr = none */
const char *quic_packet_fault(const ptls_hip_quic_packet_t &p, bool open);

/* a copy-transport slice of packets [i, s.j): plan_copy_slice over the packets' records (the cut also ends after
 * slot_max_masks packets), then what only QUIC needs.  s.gaps / s.gap_src continue behind the gaps proper with, seal: every
 * packet's header (pn_offset + pn_len bytes of h_pkt, which the record kernel reads as the AAD from the output staging);
 * open: the last 3 bytes of every plaintext area (bytes of h_out the kernel may leave unwritten, which the copies back,
 * planned for pn_len = 1, would otherwise fill with stale staging).  Gaps, headers and tails together fit the gap staging
 * (slice_bytes) whenever the packets and the areas are disjoint; EINVAL where they are not and it overflows. */
struct QuicSlicePlan {
    SlicePlan s;
    std::vector<ptls_hip_quic_packet_t> pkts; /* slice-local packet descriptors */
    std::vector<HdrDst> hdr_dst;              /* open: where the packed header entry of slice packet t goes in h_pkt */
};
int plan_quic_slice(const ptls_hip_quic_packet_t *pkts, const ptls_hip_record_t *recs, const ptls_hip_supp_t *supp, size_t n,
                    size_t i, const ModeInfo &m, size_t slice_bytes, size_t max_recs, const CopyOrder &o, QuicSlicePlan &pl);

/* ---- batch.cpp ---- */
/* one asynchronous seal / open launch of a planned batch (the device-resident calls and the TLS 1.3 ones), with the
 * kernel of the keyset's algorithm; algo != 0: the keyset (and the header-protection keyset) must be of that algorithm */
int run_batch(ptls_hip_batch_t *b, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out, uint64_t *result,
              void *stream, bool open, ptls_hip_keyset_t *hp_ks = nullptr, const ptls_hip_supp_t *supp = nullptr,
              void *mask = nullptr, int algo = 0);

/* what one seal / open launch reads of a plan, wherever the plan was made: a batch's (run_batch), the device-made one of
 * the QUIC receive step (quic_rx.cpp), which has no ptls_hip_batch_t and no host mirror of its descriptors, or a pipeline
 * slice's in its slot (pipeline.cpp).  (The descriptors are not const: the QUIC open header step, quic_unprotect, rewrites
 * them on the stream before the launch.) */
struct LaunchPlan {
    ptls_hip_engine_t *eng;
    size_t n;
    ptls_hip_record_t *d_recs;
    ptls_hip_record_t *d_recs_ord; /* plan order, or nullptr: d_recs serves as both and d_order is nullptr */
    const uint32_t *d_order;
    const Chunk *d_chunks; /* AES-GCM only, as nchunks, lanes and wg: the ChaCha kernels take the records in descriptor order */
    uint32_t nchunks;
    int lanes, wg, chacha_lanes;
    bool chacha_runs; /* ChaCha: chacha_runs_kernel.hip (launch_chacha_runs), not chacha_kernel.hip's (launch_chacha_batch) */
    bool all_aligned; /* offsets_aligned of the descriptors; the launch adds the alignment of the bases it is given */
    unsigned ncus;   /* CUs the launch is sized for (batch_cus) */
    uint64_t *d_clk; /* diagnostic clock stamps, or nullptr */
    size_t clk_bytes;
};
/* the launch of run_batch behind its refusals: n != 0, non-null buffers, every key slot inside the keyset: the kernel of
 * the keyset's algorithm with the plan's arrays, aligned when the plan is and in / aad / out are (aad == nullptr: none, the
 * kernels get `in`).  It notes no use: for a caller that waits for the stream itself (the pipelines) */
int launch_plan(const LaunchPlan &p, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out, uint64_t *result,
                void *stream, bool open, ptls_hip_keyset_t *hp_ks = nullptr, const ptls_hip_supp_t *supp = nullptr,
                void *mask = nullptr);
/* launch_plan, then the use of the keysets is noted; the caller notes the use of whatever owns the plan */
int run_plan(const LaunchPlan &p, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out, uint64_t *result, void *stream,
             bool open, ptls_hip_keyset_t *hp_ks = nullptr, const ptls_hip_supp_t *supp = nullptr, void *mask = nullptr);

/* ---- quic_parse.cpp: the steps of the parse call, shared with the receive object of quic_rx.cpp ---- */
/* the refusals of ptls_hip_quic_parse_datagrams behind its null-pointer checks */
int quic_parse_check(const char *who, ptls_hip_engine_t *eng, const ptls_hip_quic_parse_params_t *pr, ptls_hip_quic_cidmap_t *map,
                     const ptls_hip_quic_datagram_t *dgrams, size_t n, size_t buf_len);
/* n != 0: uploads the datagram array into d_dgrams, counts and scans into d_levels (scan_levels(n).words uint32), reads the
 * number of entries back into *total (synchronises the stream); mark(0) / mark(1) are called around the device work */
int quic_parse_count(const char *who, ptls_hip_engine_t *eng, const ptls_hip_quic_parse_params_t *pr, ptls_hip_quic_cidmap_t *map,
                     const ptls_hip_quic_datagram_t *dgrams, size_t n, const void *d_buf, void *d_dgrams, uint32_t *d_levels,
                     void *stream, QuicParseArgs &a, unsigned *walk_grid, uint32_t *total, const std::function<void(int)> &mark);
/* the write pass of the entries counted by quic_parse_count into device arrays of *total entries */
int quic_parse_write(const char *who, ptls_hip_quic_cidmap_t *map, QuicParseArgs &a, unsigned walk_grid, ptls_hip_quic_packet_t *d_pkts,
                     ptls_hip_quic_pktinfo_t *d_info, void *stream);

/* ---- quic.cpp ---- */
/* the lanes the inner batch of a QUIC batch was planned with (the AES batch kernel's, the ChaCha kernel's) */
void quic_batch_lanes(ptls_hip_quic_batch_t *q, int *lanes, int *chacha_lanes);
/* The header steps of n packets d_pkts in the buffer pkt, on `stream`; both return 0 or the launch's hipError_t and note no
 * use.  Open (quic_unprotect_kernel, before the record open): hp_ks's algorithm and key size give the kernel; it writes
 * the packet numbers to pn_out and the real descriptors to the record plan's d_recs, and to d_recs_ord through d_order
 * where the plan has an order.  The three are taken as they are (null order: plan position = index; pn_out and d_recs are
 * indexed by packet).  With ph, quic_unprotect_phase_kernel: the record's key slot by the Key Phase bit (quic_phase.h) and the
 * generation into ph->gen_out, indexed like pn_out.  Seal (quic_protect_kernel, behind the record seal that wrote the 16-byte
 * masks d_mask). */
int quic_unprotect(ptls_hip_engine_t *eng, const ptls_hip_keyset_t *hp_ks, const ptls_hip_quic_packet_t *d_pkts, size_t n,
                   ptls_hip_record_t *d_recs, ptls_hip_record_t *d_recs_ord, const uint32_t *d_order, void *pkt, uint64_t *pn_out,
                   void *stream, const QuicPhaseArgs *ph = nullptr);
int quic_protect(const ptls_hip_quic_packet_t *d_pkts, size_t n, void *pkt, const uint8_t *d_mask, void *stream);

/* ---- plugin_worker.cpp ---- */
/* ptls_hip_keyset_free of a plugin context's pooled slot */
void pool_release(ptls_hip_keyset_t *ks);

#pragma GCC visibility pop

#endif
