/*
 * ptls_hip.h -- MI355X (gfx950) AES-GCM record-protection engine for picotls.
 *
 * Two faces, one library (libptls_hip.so):
 *
 * 1. The picotls plugin surface.  `ptls_hip_aes128gcm` / `ptls_hip_aes256gcm` are ordinary
 *    `ptls_aead_algorithm_t` objects, interchangeable with `ptls_fusion_aes128gcm` /
 *    `ptls_fusion_aes256gcm` (reference: lib/fusion.c:1231-1256, include/picotls/fusion.h:104).
 *    Create contexts with picotls's own `ptls_aead_new` / `ptls_aead_new_direct`
 *    (lib/picotls.c:6452-6473) and use `ptls_aead_encrypt*` / `ptls_aead_decrypt`
 *    (include/picotls.h:1993-2055).  Each call is synchronous and runs one record on the GPU.
 *
 * 2. The batch extension (picotls has no batch API).  Many independent records, each with its own
 *    key slot, sequence number, AAD, input and output, are sealed or opened by one asynchronous
 *    kernel launch on a HIP stream.  Inputs and outputs are device pointers.  This is the
 *    throughput path measured by bench.py.
 *
 * Plain C ABI: pointers, sizes, integers.  `stream` is a hipStream_t passed as void* (NULL = the
 * null stream).  Functions returning int give 0 on success and a negative PTLS_HIP_E* code on
 * failure; `ptls_hip_last_error()` describes the most recent failure on the calling thread.
 */
#ifndef PTLS_HIP_H
#define PTLS_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "picotls_plugin_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTLS_HIP_EINVAL (-1)   /* bad argument */
#define PTLS_HIP_ENODEV (-2)   /* no usable gfx950 device / HIP runtime failure */
#define PTLS_HIP_ENOMEM (-3)   /* device or host allocation failed */
#define PTLS_HIP_ELAUNCH (-4)  /* kernel launch failed */

const char *ptls_hip_last_error(void);

/* ------------------------------------------------------------------------------------------ *
 * 1. picotls plugin objects                                                                   *
 * ------------------------------------------------------------------------------------------ */

/* Replace ptls_fusion_aes128gcm / ptls_fusion_aes256gcm (lib/fusion.c:1231-1256).
 * setup_crypto returns non-zero (=> ptls_aead_new returns NULL) when no gfx950 device is usable;
 * key == NULL re-sets the static IV only (as fusion's aesgcm_setup, lib/fusion.c:1188-1191).
 * do_encrypt / do_encrypt_v / do_decrypt match lib/fusion.c:1135-1166 byte for byte, and in
 * addition implement do_encrypt_v (fusion asserts "FIXME" there, lib/fusion.c:1145-1149). */
extern ptls_aead_algorithm_t ptls_hip_aes128gcm, ptls_hip_aes256gcm;

/* Replace ptls_non_temporal_aes128gcm / ptls_non_temporal_aes256gcm (lib/fusion.c:2109-2179): the same
 * field values (TLS 1.2 IV sizes {4, 8}, non_temporal = 1, align_bits = 6) and the same per-direction
 * vtable (is_enc: do_encrypt + do_encrypt_v, no do_decrypt; otherwise do_decrypt only; init/update/final
 * NULL).  Output bytes equal the fusion AEAD's, as the reference's own are. */
extern ptls_aead_algorithm_t ptls_hip_non_temporal_aes128gcm, ptls_hip_non_temporal_aes256gcm;

/* Replace ptls_fusion_aes128ctr / ptls_fusion_aes256ctr (lib/fusion.c:1050-1100, :1219-1230), the
 * `ctr_cipher` of the AEAD objects above and the cipher QUIC stacks use for header protection.
 * Same contract as fusion's: do_init(iv) computes one keystream block AES-ECB(key, iv) on the GPU, and
 * the following do_transform XORs at most 16 bytes with it (fusion asserts the same, :1064-1077).
 * When such a context is passed as `supp` to ptls_hip_aes*gcm's do_encrypt (ptls_aead_encrypt_s),
 * the mask is computed inside the same kernel launch as the record, as fusion does (:636-650). */
extern ptls_cipher_algorithm_t ptls_hip_aes128ctr, ptls_hip_aes256ctr;

/* Replace ptls_minicrypto_chacha20poly1305 / ptls_minicrypto_chacha20 (lib/cifra/chacha20.c:97-113; the OpenSSL and
 * mbedTLS backends export the same values): TLS_CHACHA20_POLY1305_SHA256's AEAD and the ChaCha20 cipher QUIC uses for
 * header protection.  Same vtable shape as the AES objects above (do_encrypt with supp, do_encrypt_v, do_decrypt, get /
 * set IV, dispose; key == NULL re-sets the static IV only).  The cipher follows the contract of ptls_hip_aes*ctr:
 * do_init(iv16) computes one keystream block on the GPU (counter = LE32(iv[0..4]), nonce = iv[4..16]) and the following
 * do_transform XORs at most 16 bytes with it.  Every call is one kernel launch of its own; the resident worker does not
 * serve these objects (they work whatever PTLS_HIP_PLUGIN_WORKER says). */
extern ptls_aead_algorithm_t ptls_hip_chacha20poly1305;
extern ptls_cipher_algorithm_t ptls_hip_chacha20;

/* Device ordinal used by contexts created through the plugin objects (default 0; also read from
 * the environment variable PTLS_HIP_DEVICE).  Must be called before the first context is made. */
int ptls_hip_set_default_device(int device);

/* 1 when a gfx950 (MI355X) device is visible to this process, else 0: the counterpart of
 * ptls_fusion_is_supported_by_cpu (lib/fusion.c:2219-2249), for choosing the cipher suites at start-up.
 * Counts devices without creating a context. */
int ptls_hip_is_supported(void);

/* Fusion-style low-level single-record AES-GCM context (include/picotls/fusion.h:56-96,
 * lib/fusion.c:400-1048), for callers that drive fusion below the AEAD plugin (as its benchmarks and
 * tests do).  One record per call, host buffers, synchronous.
 *   nonce   the 12-byte GCM nonce (static IV xor big-endian sequence number).  Fusion takes the
 *           same value as a byte-swapped __m128i counter block (calc_counter, lib/fusion.c:1126-1133),
 *           which is x86-only; the nonce bytes are the portable form of it.
 *   capacity  maximum AAD + payload size, as fusion's; staging also grows on demand, and
 *           set_capacity returns the same context.
 * encrypt writes inlen bytes of ciphertext followed by the 16-byte tag.  supp (optional) is handled as
 * by the AEAD plugin's do_encrypt.  decrypt reads inlen bytes of ciphertext and the detached 16-byte
 * tag, always writes inlen bytes of plaintext, and returns 1 when the tag matches and 0 otherwise
 * (lib/fusion.c:660-...).  new returns NULL for a key size other than 16 or 32, or without a device. */
typedef struct ptls_hip_aesgcm_context ptls_hip_aesgcm_context_t;
ptls_hip_aesgcm_context_t *ptls_hip_aesgcm_new(const void *key, size_t key_size, size_t capacity);
ptls_hip_aesgcm_context_t *ptls_hip_aesgcm_set_capacity(ptls_hip_aesgcm_context_t *ctx, size_t capacity);
void ptls_hip_aesgcm_free(ptls_hip_aesgcm_context_t *ctx);
void ptls_hip_aesgcm_encrypt(ptls_hip_aesgcm_context_t *ctx, void *output, const void *input, size_t inlen, const void *nonce,
                             const void *aad, size_t aadlen, ptls_aead_supplementary_encryption_t *supp);
int ptls_hip_aesgcm_decrypt(ptls_hip_aesgcm_context_t *ctx, void *output, const void *input, size_t inlen, const void *nonce,
                            const void *aad, size_t aadlen, const void *tag);

/* Fusion's public one-block AES-ECB API (ptls_fusion_aesecb_init / _dispose / _encrypt,
 * include/picotls/fusion.h:52-54, lib/fusion.c:857-928): an encryption-only AES-128/256 key schedule and
 * single-block encryption, here with the key expanded into a device key slot and each block encrypted by
 * one kernel launch (synchronous, host buffers).  Same arguments as fusion's, including the trailing
 * `aesni256` (an x86 code-path switch there, ignored here).  Fusion's init returns void and asserts on
 * decryption or a key size other than 16 / 32; this one returns 0, or PTLS_HIP_EINVAL for those cases and
 * PTLS_HIP_ENODEV without a usable gfx950 device (ctx->state is then NULL and dispose is a no-op).
 * dispose zeroizes and releases the device key slot. */
typedef struct st_ptls_hip_aesecb_context_t {
    void *state;     /* engine-owned: key slot, staging, stream */
    unsigned rounds; /* 10 or 14, as fusion's ctx->rounds */
} ptls_hip_aesecb_context_t;
int ptls_hip_aesecb_init(ptls_hip_aesecb_context_t *ctx, int is_enc, const void *key, size_t key_size, int aesni256);
void ptls_hip_aesecb_dispose(ptls_hip_aesecb_context_t *ctx);
void ptls_hip_aesecb_encrypt(ptls_hip_aesecb_context_t *ctx, void *dst, const void *src);

/* ------------------------------------------------------------------------------------------ *
 * 2. batch extension                                                                          *
 * ------------------------------------------------------------------------------------------ */

typedef struct st_ptls_hip_engine_t ptls_hip_engine_t;
typedef struct st_ptls_hip_keyset_t ptls_hip_keyset_t;
typedef struct st_ptls_hip_batch_t ptls_hip_batch_t;

/* One engine per device: owns the device's AES tables and the launch configuration. */
ptls_hip_engine_t *ptls_hip_engine_new(int device);
void ptls_hip_engine_free(ptls_hip_engine_t *engine);
int ptls_hip_engine_device(ptls_hip_engine_t *engine);
int ptls_hip_engine_cu_count(ptls_hip_engine_t *engine);

/* A keyset is an array of device-resident AEAD contexts ("key slots"), all AES-128 (key_size 16)
 * or all AES-256 (key_size 32).  Slot i corresponds to one ptls_aead_context_t of the plugin
 * surface: key schedule, GHASH key powers and the 12-byte static IV. */
ptls_hip_keyset_t *ptls_hip_keyset_new(ptls_hip_engine_t *engine, size_t key_size, size_t nslots);
void ptls_hip_keyset_free(ptls_hip_keyset_t *ks); /* zeroizes device key material */
size_t ptls_hip_keyset_size(ptls_hip_keyset_t *ks);
/* The AEAD of a keyset.  ptls_hip_keyset_new makes AES-GCM keysets; ptls_hip_keyset_new_algo takes the algorithm:
 * PTLS_HIP_ALGO_AESGCM with key_size 16 or 32 (the same keyset ptls_hip_keyset_new makes), or
 * PTLS_HIP_ALGO_CHACHA20POLY1305 with key_size 32 (TLS_CHACHA20_POLY1305_SHA256; as a header-protection keyset: QUIC's
 * ChaCha20 header protection).  A ChaCha slot is the 32-byte key and the 12-byte static IV, 44 bytes of device memory:
 * nothing is expanded.  keyset_set / get_iv / set_iv / xor_iv / set_secrets / update_secrets (hash_size 32) / free work on
 * both kinds; seal / open calls take the kind their name says (2a below) and fail with PTLS_HIP_EINVAL, launching
 * nothing, on the other; the TLS 1.3 calls (2b) take either.  A host pipeline (2c) serves the algorithm it was made for
 * (ptls_hip_pipeline_new_algo); nodes (2d) are AES-GCM only. */
#define PTLS_HIP_ALGO_AESGCM 1
#define PTLS_HIP_ALGO_CHACHA20POLY1305 2
ptls_hip_keyset_t *ptls_hip_keyset_new_algo(ptls_hip_engine_t *engine, int algo, size_t key_size, size_t nslots);
int ptls_hip_keyset_algo(ptls_hip_keyset_t *ks);
/* Load `count` keys (count * key_size bytes) and static IVs (count * 12 bytes; NULL = zero IVs, e.g. for
 * header-protection keys) from host memory into slots [first, first + count) and expand them on the
 * device (key schedule, H = E_K(0), powers of H).
 * Equivalent to setup_crypto(ctx, is_enc, key, iv) for each slot (lib/fusion.c:1184-1206). */
int ptls_hip_keyset_set(ptls_hip_keyset_t *ks, size_t first, size_t count, const void *keys, const void *ivs, void *stream);
/* Static-IV get/set of one slot (do_get_iv / do_set_iv, lib/fusion.c:1168-1182); with
 * ptls_hip_keyset_xor_iv this gives ptls_aead_xor_iv semantics (lib/picotls.c:6481-6490). */
int ptls_hip_keyset_get_iv(ptls_hip_keyset_t *ks, size_t slot, void *iv);
int ptls_hip_keyset_set_iv(ptls_hip_keyset_t *ks, size_t slot, const void *iv, void *stream);
int ptls_hip_keyset_xor_iv(ptls_hip_keyset_t *ks, size_t slot, const void *bytes, size_t len, void *stream);

/* Many-connection key management, on the device.  `secrets` = count TLS 1.3
 * traffic secrets of hash_size bytes (32: SHA-256 suites, 48: SHA-384) in host memory.
 * set_secrets: slot i gets the record key / IV picotls derives from secret i when it creates the
 *   connection's AEAD (HKDF-Expand-Label "key" / "iv", get_traffic_keys, lib/picotls.c:1603-1622).
 * update_secrets: the TLS 1.3 key update (update_traffic_key, lib/picotls.c:4980-4996): every secret
 *   becomes HKDF-Expand-Label(secret, "traffic upd", "", hash_size) -- written back to `secrets` -- and the
 *   slots are re-keyed from the new secrets.  Both run one device thread per connection. */
int ptls_hip_keyset_set_secrets(ptls_hip_keyset_t *ks, size_t first, size_t count, const void *secrets, size_t hash_size,
                                void *stream);
int ptls_hip_keyset_update_secrets(ptls_hip_keyset_t *ks, size_t first, size_t count, void *secrets, size_t hash_size,
                                   void *stream);

/* Record descriptor (48 bytes).  Offsets are byte offsets into the buffers passed to seal/open.
 *   seal: reads len bytes at in+in_off, writes len bytes of ciphertext and the 16-byte tag at
 *         out+out_off (len + 16 bytes), like ptls_aead_encrypt (include/picotls.h:1993).
 *   open: reads len bytes of ciphertext followed by the 16-byte tag at in+in_off, writes len bytes
 *         of plaintext at out+out_off (always, like fusion's decrypt-then-verify), and sets
 *         result[i] = len on success or UINT64_MAX on authentication failure (the SIZE_MAX of
 *         ptls_aead_decrypt, lib/fusion.c:1151-1166).
 * The nonce is slot.iv with bytes 4..11 XORed with big-endian seq (ptls_aead__build_iv,
 * lib/picotls.c:6492-6506).  in == out (in place) is allowed.  For full speed keep in_off, out_off
 * 16-byte aligned and put records of the same key next to each other.  The kernels read exactly the
 * record's input (+ tag on open) and AAD bytes and write exactly its output bytes: buffers need no padding
 * past the last record (partial blocks are loaded as whole dwords + single bytes). */
typedef struct st_ptls_hip_record_t {
    uint64_t in_off;
    uint64_t out_off;
    uint64_t aad_off;
    uint64_t seq;
    uint32_t len;
    uint32_t aad_len;
    uint32_t key;   /* key slot index */
    uint32_t flags; /* 0, or PTLS_HIP_RECORD_TLS13_TYPE(type) (seal: TLS 1.3 inner content type, see 2c) */
} ptls_hip_record_t;
/* seal only: the record's plaintext is the len - 1 input bytes followed by the content-type byte `type`
 * (TLSInnerPlaintext without padding, RFC 8446 §5.2; picotls's aead_encrypt, lib/picotls.c:705-715) */
#define PTLS_HIP_RECORD_TLS13_TYPE(type) (1u | ((uint32_t)(uint8_t)(type) << 8))

/* Upload `n` host descriptors and plan the launch (runs of equal key slot, lane-group width from the
 * record lengths).  A batch is reusable for any number of seal/open calls over same-shaped buffers. */
ptls_hip_batch_t *ptls_hip_batch_new(ptls_hip_engine_t *engine, const ptls_hip_record_t *recs, size_t n, void *stream);
void ptls_hip_batch_free(ptls_hip_batch_t *batch);
size_t ptls_hip_batch_count(ptls_hip_batch_t *batch);
/* lanes cooperating on one record (1, 2, 4, 8, 16 or 32), or 64: one wave per record with key-independent
 * LDS (the kernel chosen for batches of many keys with few records each); 0 = automatic (default). */
int ptls_hip_batch_set_lanes(ptls_hip_batch_t *batch, int lanes);
int ptls_hip_batch_lanes(ptls_hip_batch_t *batch);
/* threads per workgroup of the batch kernel (512 or 768); 0 = automatic (default).  For tuning. */
int ptls_hip_batch_set_workgroup(ptls_hip_batch_t *batch, int threads);
int ptls_hip_batch_workgroup(ptls_hip_batch_t *batch);
/* at most `n` workgroups per launch, and chunks planned as for a device of n CUs (0 = the device's CU
 * count, the default).  For tests of the work distribution (a workgroup then takes several chunks of one
 * key run) and for sharing a device with other work. */
int ptls_hip_batch_set_max_workgroups(ptls_hip_batch_t *batch, int n);
/* chunks of the launch plan (runs of one key slot, at most 32 wave tasks each; the sparse kernel's plan: one) */
int ptls_hip_batch_chunks(ptls_hip_batch_t *batch);
/* workgroups one seal/open launch of the batch uses (for sizing the clock-stamp buffer below) */
int ptls_hip_batch_grid(ptls_hip_batch_t *batch);
/* Diagnostic: the following launches of the batch write, per workgroup w, the shader-cycle counter and the constant
 * 100 MHz counter at the start and at the end of its work: d_buf[4w .. 4w + 3] = {cycles0, ticks0, cycles1, ticks1}
 * (uint64, device memory of >= 32 bytes per workgroup).  delta(cycles) / delta(ticks) x 100 MHz = the clock the launch
 * ran at.  d_buf == NULL switches the stamps off (the default: then no stamp instruction executes). */
int ptls_hip_batch_set_clock(ptls_hip_batch_t *batch, void *d_buf, size_t nbytes);

/* Asynchronous on `stream`; all pointers are device (or device-accessible) memory.  Fails with
 * PTLS_HIP_EINVAL (nothing launched) when a record names a key slot outside `ks`. */
int ptls_hip_aesgcm_seal_batch(ptls_hip_batch_t *batch, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out,
                               void *stream);
int ptls_hip_aesgcm_open_batch(ptls_hip_batch_t *batch, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out,
                               uint64_t *result, void *stream);

/* QUIC header protection for a batch (RFC 9001 §5.4; fusion's `supp`, lib/fusion.c:424-428, :636-650).
 * One descriptor per record (same index as the batch's descriptors): mask + mask_off receives the
 * 16-byte AES-ECB(hp key slot `hp_key`, 16 bytes at sample_off) -- for seal the sample is read from
 * `out` AFTER the record (ciphertext and tag) is written, so it may cover the tag, exactly like
 * fusion's supplementary block.  Records with (flags & 1) == 0, or whose hp_key is outside the
 * header-protection keyset (the descriptors are device data, so this is checked on the device), are
 * skipped and their mask bytes left untouched.  The header-protection
 * keyset must have the AEAD keyset's key size (fusion runs the supp block with the AEAD's rounds). */
typedef struct st_ptls_hip_supp_t {
    uint64_t sample_off;
    uint64_t mask_off;
    uint32_t hp_key;
    uint32_t flags;
} ptls_hip_supp_t;
#define PTLS_HIP_SUPP_ENABLE 1u

/* seal_batch + header-protection masks in the same launch; `supp` is a device array of batch_count. */
int ptls_hip_aesgcm_seal_batch_supp(ptls_hip_batch_t *batch, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                    const ptls_hip_supp_t *supp, const void *in, const void *aad, void *out, void *mask,
                                    void *stream);
/* Standalone masks (receive side: the sample is ciphertext in the received packet, needed before the
 * packet number can be read and the record opened): mask + mask_off = AES-ECB(hp key, src + sample_off)
 * for n device descriptors. */
int ptls_hip_aesecb_batch(ptls_hip_engine_t *engine, ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp, size_t n,
                          const void *src, void *mask, void *stream);

/* ------------------------------------------------------------------------------------------ *
 * 2a. ChaCha20-Poly1305 (RFC 8439 §2.8; picotls lib/chacha20poly1305.h) over the same batches    *
 * ------------------------------------------------------------------------------------------ */

/* The same descriptors with the same meaning as the aesgcm calls above (nonce, in place, exact bytes, result, the TLS 1.3
 * content-type flag), on a keyset of PTLS_HIP_ALGO_CHACHA20POLY1305.  Records are taken in descriptor order: there is no
 * per-key state to share, so batches of many keys cost nothing extra.  PTLS_HIP_EINVAL (nothing launched) on an AES keyset
 * or when a record names a key slot outside `ks`. */
int ptls_hip_chacha20poly1305_seal_batch(ptls_hip_batch_t *batch, ptls_hip_keyset_t *ks, const void *in, const void *aad,
                                         void *out, void *stream);
int ptls_hip_chacha20poly1305_open_batch(ptls_hip_batch_t *batch, ptls_hip_keyset_t *ks, const void *in, const void *aad,
                                         void *out, uint64_t *result, void *stream);
/* seal + QUIC ChaCha20 header-protection masks in the same launch (RFC 9001 §5.4.4): for enabled descriptors, sample = the
 * 16 bytes at out + sample_off after the record is written, and mask + mask_off receives the first 16 keystream bytes of
 * ChaCha20(hp key, counter = LE32(sample[0..4]), nonce = sample[4..16]) -- what ptls_aead__do_encrypt produces with a
 * ptls_minicrypto_chacha20 supp context (include/picotls.h:2027-2038, lib/cifra/chacha20.c:44-56); QUIC uses the first 5.
 * hp_ks is a ChaCha keyset too (its IVs are not used).  Skipped descriptors leave their mask bytes untouched. */
int ptls_hip_chacha20poly1305_seal_batch_supp(ptls_hip_batch_t *batch, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                              const ptls_hip_supp_t *supp, const void *in, const void *aad, void *out,
                                              void *mask, void *stream);
/* standalone masks for n device descriptors (the receive side), the counterpart of ptls_hip_aesecb_batch */
int ptls_hip_chacha20_mask_batch(ptls_hip_engine_t *engine, ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp, size_t n,
                                 const void *src, void *mask, void *stream);
/* lanes cooperating on one record in the ChaCha kernel: 1, 4, 16 or 64; 0 = automatic from the record lengths (default) */
int ptls_hip_batch_set_chacha_lanes(ptls_hip_batch_t *batch, int lanes);
int ptls_hip_batch_chacha_lanes(ptls_hip_batch_t *batch);

/* ------------------------------------------------------------------------------------------ *
 * 2b. TLS 1.3 record layer over the batch                      *
 * ------------------------------------------------------------------------------------------ */

#define PTLS_HIP_TLS13_MAX_PLAINTEXT 16384         /* PTLS_MAX_PLAINTEXT_RECORD_SIZE, lib/picotls.c:42 */
#define PTLS_HIP_TLS13_MAX_ENCRYPTED (16384 + 256) /* PTLS_MAX_ENCRYPTED_RECORD_SIZE, lib/picotls.c:43 */
/* wire bytes of one message of `len` payload bytes: ceil(len / 16384) records of 5 + chunk + 1 + 16 */
size_t ptls_hip_tls13_wire_size(size_t len);

/* Send side.  A message = `len` bytes of one content type for one connection (key slot); like
 * buffer_push_encrypted_records (lib/picotls.c:747-794) it is cut into records of at most 16384 bytes,
 * record j carrying seq + j, all written back to back at out + out_off as
 *     17 03 03 BE16(chunk + 17) || AES-GCM(chunk || type, AAD = that 5-byte header) || tag
 * (build_aad and aead_encrypt, lib/picotls.c:696-715).  len == 0 produces no record. */
typedef struct st_ptls_hip_tls13_message_t {
    uint64_t in_off;  /* payload in the `in` buffer */
    uint64_t out_off; /* first wire byte in the `out` buffer */
    uint64_t seq;     /* sequence number of the first record */
    uint32_t len;
    uint32_t key;  /* key slot */
    uint32_t type; /* content type (PTLS_CONTENT_TYPE_APPDATA = 23, handshake 22, alert 21) */
    uint32_t reserved;
} ptls_hip_tls13_message_t;
/* Host-side planning: fills up to `cap` record descriptors (aad_off = header position in `out`) and
 * returns the number of records the messages need (call with recs == NULL to size the array). */
size_t ptls_hip_tls13_frame(const ptls_hip_tls13_message_t *msgs, size_t n, ptls_hip_record_t *recs, size_t cap);
/* Writes the record headers into `out`, then seals every record (AAD read from the headers). */
int ptls_hip_tls13_seal_batch(ptls_hip_batch_t *batch, ptls_hip_keyset_t *ks, const void *in, void *out, void *stream);

/* Receive side.  Parses complete TLS records from a received byte stream on the host, like picotls's
 * parse_record / parse_record_header (lib/picotls.c:5020-5062): application-data records (type 23) of 16 to
 * 16384 + 256 bytes become descriptors {aad_off = header, in_off = header + 5, len = length - 16,
 * seq = seq + i, key, out_off = out_base + plaintext position}, at most `cap` of them (recs may be NULL
 * when cap is 0).  Stops before the first incomplete record, record of another type (change_cipher_spec,
 * alert, handshake) or record whose legacy_record_version is not 03 03: the caller's picotls record layer
 * handles those (ptls_receive from *consumed on); *consumed = wire bytes of the records
 * produced, *nrecs = their number.  Returns 0; or PTLS_HIP_TLS13_DECODE_ERROR for a byte that is no record
 * type or an oversized application-data record (as parse_record); or PTLS_HIP_TLS13_SHORT_RECORD for a
 * complete application-data record shorter than a tag (picotls's aead_decrypt fails it with
 * PTLS_ALERT_BAD_RECORD_MAC, :717-726).  The records before the error are produced either way. */
#define PTLS_HIP_TLS13_DECODE_ERROR (-50) /* -PTLS_ALERT_DECODE_ERROR */
#define PTLS_HIP_TLS13_SHORT_RECORD (-20) /* -PTLS_ALERT_BAD_RECORD_MAC */
int ptls_hip_tls13_parse(const void *wire, size_t wire_len, uint64_t wire_off, uint32_t key, uint64_t seq, uint64_t out_base,
                         ptls_hip_record_t *recs, size_t cap, size_t *nrecs, size_t *consumed);
/* Opens the records (AAD = their wire headers in `in`), strips the TLSInnerPlaintext padding and reads
 * the content type, like handle_input (lib/picotls.c:5866-5883).  result[i] = content length |
 * (uint64_t)type << 56, or PTLS_HIP_TLS13_BAD_RECORD_MAC (authentication failure), or
 * PTLS_HIP_TLS13_NO_CONTENT_TYPE (all-zero plaintext: PTLS_ALERT_UNEXPECTED_MESSAGE in picotls). */
#define PTLS_HIP_TLS13_BAD_RECORD_MAC UINT64_MAX
#define PTLS_HIP_TLS13_NO_CONTENT_TYPE (UINT64_MAX - 1)
int ptls_hip_tls13_open_batch(ptls_hip_batch_t *batch, ptls_hip_keyset_t *ks, const void *in, void *out, uint64_t *result,
                              void *stream);

/* ------------------------------------------------------------------------------------------ *
 * 2c. host-resident records (records arrive in and leave through host memory: socket buffers)  *
 * ------------------------------------------------------------------------------------------ */

/* A pipeline owns three device staging slots of `slice_bytes` each and three streams.  seal/open
 * cut the record list into slices whose input / output / AAD byte spans fit a slot and overlap, per
 * slice, H2D copy -> kernel -> D2H copy.  Offsets in `recs` are relative to the host buffers.  The
 * call returns when every output byte (and result) is in host memory.  Host buffers should be
 * pinned (hipHostMalloc'd, or ptls_hip_host_register'ed) for the copies to run asynchronously.
 * Only the records' output bytes change in the caller's output buffer (as fusion's storen128 and tag
 * store, lib/fusion.c:388-397, :632): a slice's output comes back as the records' runs, several runs
 * joined by one copy over short gaps that were first filled, on the device, with the caller's own bytes
 * of those gaps (read when the slice is planned; do not modify them during the call), never over another
 * slice's record.  The masks of seal_supp are written packed into the slice's staging, come back by one
 * copy per slice and are placed at their mask_off by the host: no other byte of h_mask is read or written,
 * the masks of a slice may lie anywhere in h_mask (between other slices' masks too), and a slice ends
 * after slice_bytes / 64 masks.  Whole QUIC packets, header protection included, go through the same pipelines with
 * ptls_hip_pipeline_quic_seal / _open (2g). */
typedef struct st_ptls_hip_pipeline_t ptls_hip_pipeline_t;
ptls_hip_pipeline_t *ptls_hip_pipeline_new(ptls_hip_engine_t *engine, size_t slice_bytes);
void ptls_hip_pipeline_free(ptls_hip_pipeline_t *p);
int ptls_hip_pipeline_seal(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                           const void *h_in, const void *h_aad, void *h_out);
int ptls_hip_pipeline_open(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                           const void *h_in, const void *h_aad, void *h_out, uint64_t *h_result);
/* seal + QUIC header-protection masks from and to host memory: `supp` is a HOST array indexed like recs
 * (offsets relative to h_out / h_mask); every enabled sample must lie inside the output of the records
 * sealed with it (QUIC: pn_offset + 4 is in the ciphertext).  Masks are written at h_mask + mask_off;
 * other bytes of h_mask are preserved. */
int ptls_hip_pipeline_seal_supp(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                const ptls_hip_record_t *recs, const ptls_hip_supp_t *supp, size_t n, const void *h_in,
                                const void *h_aad, void *h_out, void *h_mask);
/* The TLS 1.3 record layer from and to host memory (socket buffers): `recs` from ptls_hip_tls13_frame
 * (seal: h_in holds the messages, h_wire receives header + ciphertext + tag of every record) or from
 * ptls_hip_tls13_parse (open: h_wire is the received stream, h_out receives the inner content, h_result
 * is as in ptls_hip_tls13_open_batch).  Same slicing and overlap as ptls_hip_pipeline_seal/open. */
int ptls_hip_pipeline_tls13_seal(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                                 const void *h_in, void *h_wire);
int ptls_hip_pipeline_tls13_open(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, const ptls_hip_record_t *recs, size_t n,
                                 const void *h_wire, void *h_out, uint64_t *h_result);
/* How a pipeline moves the bytes.  AUTO (the default): MAPPED when every host buffer of the call (in, out, aad,
 * mask) is pinned or registered, COPY otherwise.  COPY: the staging described above (copy engines).  MAPPED: no
 * staging -- the kernels read the records from and write them to the host buffers over PCIe themselves (their
 * device mappings, hipHostGetDevicePointer), one launch per max-records slice; bytes between records in the
 * output are never written, as by the device-resident batch calls.  A call in MAPPED mode with an unmapped
 * buffer fails with PTLS_HIP_EINVAL.  last_transport: what the last seal/open of the pipeline used. */
#define PTLS_HIP_TRANSPORT_AUTO 0
#define PTLS_HIP_TRANSPORT_COPY 1
#define PTLS_HIP_TRANSPORT_MAPPED 2
int ptls_hip_pipeline_set_transport(ptls_hip_pipeline_t *p, int transport);
int ptls_hip_pipeline_last_transport(ptls_hip_pipeline_t *p);
/* The algorithm a pipeline serves is fixed when it is made.  ptls_hip_pipeline_new makes AES-GCM pipelines, and so does
 * ptls_hip_pipeline_new_algo with PTLS_HIP_ALGO_AESGCM (the same object); with PTLS_HIP_ALGO_CHACHA20POLY1305 it makes a
 * pipeline for ChaCha20-Poly1305 keysets: the five calls above on both transports, with the argument rules, buffer checks and
 * exact-bytes promises above; seal_supp takes a ChaCha header-protection keyset and writes the masks of
 * ptls_hip_chacha20poly1305_seal_batch_supp.  Any other algo: NULL.  A call with a keyset (or header-protection keyset) of
 * the other algorithm fails with PTLS_HIP_EINVAL and touches nothing. */
ptls_hip_pipeline_t *ptls_hip_pipeline_new_algo(ptls_hip_engine_t *engine, int algo, size_t slice_bytes);
int ptls_hip_pipeline_algo(ptls_hip_pipeline_t *p);
/* For tests and tuning, on a ChaCha pipeline (PTLS_HIP_EINVAL on an AES-GCM one): the lanes per record of the slices' record
 * kernel (0 = automatic, 1, 4, 16, 64) and how they move a record's whole 64-byte blocks.  BLOCKS: a lane loads and stores its
 * own block, the kernel of the device-resident calls (2a).  RUNS (4 lanes or more): instruction j of a lane group moves the
 * contiguous 16 x lanes bytes j of the group's 64 x lanes, and the lanes exchange the pieces inside quads; made for host
 * memory, where the run length per instruction matters.  AUTO, as measured: on the mapped transport RUNS at
 * 64 lanes for slices whose mean record has 64 whole blocks or more, BLOCKS at 64 or 16 lanes for shorter ones; BLOCKS on
 * the copy transport's device staging.  Both layouts compute the same bytes. */
#define PTLS_HIP_CHACHA_LAYOUT_AUTO 0
#define PTLS_HIP_CHACHA_LAYOUT_BLOCKS 1
#define PTLS_HIP_CHACHA_LAYOUT_RUNS 2
int ptls_hip_pipeline_set_chacha_lanes(ptls_hip_pipeline_t *p, int lanes, int layout);
int ptls_hip_host_register(void *ptr, size_t len);
int ptls_hip_host_unregister(void *ptr);

/* ------------------------------------------------------------------------------------------ *
 * 2d. one batch over several devices (records are independent, no collective)  *
 * ------------------------------------------------------------------------------------------ */

/* Host-side planning: contiguous ranges of about equal payload bytes.  bounds (parts + 1 entries): range r =
 * records [bounds[r], bounds[r + 1]), bounds[0] = 0, bounds[parts] = n; range r ends right after the first record
 * whose prefix sum of len reaches ceil(total * (r + 1) / parts).  Equal counts for equal lengths. */
int ptls_hip_partition_bytes(const ptls_hip_record_t *recs, size_t n, size_t parts, size_t *bounds);

/* A node: one engine, one keyset (nslots key slots of key_size) and one host pipeline (slice_bytes, as
 * ptls_hip_pipeline_new) per listed device; a device may be listed more than once.  seal / open split the records by
 * ptls_hip_partition_bytes and run every range on its own device from its own host thread, through that device's
 * pipeline (transport AUTO by default: the kernels read and write pinned host buffers over the device's own PCIe link),
 * and return when every device is done.  Records, offsets and buffers are as for ptls_hip_pipeline_seal / open.
 * node_keyset_set loads the same keys into every device's keyset (ptls_hip_keyset_set semantics).
 * last_split: the last call's per-device wall-clock seconds (ndev doubles) and record ranges (ndev + 1 bounds),
 * either pointer may be NULL; whole-node rate = payload bytes / the largest of the seconds. */
typedef struct st_ptls_hip_node_t ptls_hip_node_t;
ptls_hip_node_t *ptls_hip_node_new(const int *devices, size_t ndev, size_t key_size, size_t nslots, size_t slice_bytes);
void ptls_hip_node_free(ptls_hip_node_t *node);
size_t ptls_hip_node_size(ptls_hip_node_t *node);
int ptls_hip_node_keyset_set(ptls_hip_node_t *node, size_t first, size_t count, const void *keys, const void *ivs);
int ptls_hip_node_set_transport(ptls_hip_node_t *node, int transport);
int ptls_hip_node_seal(ptls_hip_node_t *node, const ptls_hip_record_t *recs, size_t n, const void *h_in, const void *h_aad,
                       void *h_out);
int ptls_hip_node_open(ptls_hip_node_t *node, const ptls_hip_record_t *recs, size_t n, const void *h_in, const void *h_aad,
                       void *h_out, uint64_t *h_result);
int ptls_hip_node_last_split(ptls_hip_node_t *node, double *seconds, size_t *bounds);
/* NUMA placement (each GPU's records in host memory on its own NUMA node).  device_numa_node: the node
 * a device's PCI function hangs off (sysfs), -1 if unknown.  node_numa: that node for every device of the node (ndev
 * ints).  Each device's host thread runs on its node's CPUs.  node_host_alloc: `bytes` of host memory whose range
 * [splits[d], splits[d + 1]) (ndev + 1 byte offsets, 0 .. bytes; whole pages, a shared page goes with the lower range)
 * is bound to device d's node and faulted in there, registered with every device (mapped, portable) so both transports
 * use it zero-copy; released with node_host_free(ptr, bytes).  host_page_nodes: the node of every stride-th page of
 * [ptr, ptr + bytes) (move_pages), at most cap of them; returns how many were written. */
int ptls_hip_device_numa_node(int device);
int ptls_hip_node_numa(ptls_hip_node_t *node, int *numa_nodes);
void *ptls_hip_node_host_alloc(ptls_hip_node_t *node, size_t bytes, const size_t *splits);
void ptls_hip_node_host_free(void *ptr, size_t bytes);
size_t ptls_hip_host_page_nodes(const void *ptr, size_t bytes, size_t stride, int *nodes, size_t cap);

/* ------------------------------------------------------------------------------------------ *
 * 2e. QUIC packet protection (RFC 9001 §5.3, §5.4) over the same batches, packets on the device  *
 * ------------------------------------------------------------------------------------------ */

/* One QUIC packet (40 bytes).  Offsets are byte offsets into the buffers passed to the calls below; packets may lie at
 * any byte offset.  The packet is header (pn_offset bytes) || packet number (pn_len bytes) || payload || 16-byte tag. */
typedef struct st_ptls_hip_quic_packet_t {
    uint64_t pkt_off;   /* first header byte of the packet in `pkt` */
    uint64_t data_off;  /* seal: the plaintext payload in `in`; open: where the plaintext goes in `out` */
    uint64_t pn;        /* seal: the full packet number (< 2^62);
                           open: the expected one = largest packet number received in this space + 1 */
    uint32_t pkt_len;   /* whole packet: header, packet number, payload, 16-byte tag */
    uint32_t key;       /* AEAD key slot */
    uint32_t hp_key;    /* header-protection key slot */
    uint16_t pn_offset; /* header bytes in front of the packet-number field (>= 1) */
    uint8_t pn_len;     /* seal: 1..4, equal to (first byte & 3) + 1 of the header the caller wrote; open: ignored */
    uint8_t flags;      /* open: PTLS_HIP_QUIC_UNPROTECTED = the header is already unprotected (see below) */
} ptls_hip_quic_packet_t;
#define PTLS_HIP_QUIC_UNPROTECTED 1u

/* A QUIC batch: `n` host descriptors uploaded and planned for seal (open == 0) or for open (open != 0); reusable for any
 * number of calls of that direction over same-shaped buffers.  NULL (PTLS_HIP_EINVAL in ptls_hip_last_error, which names
 * the packet's index) when a packet has pn_offset == 0 or pkt_len < pn_offset + 4 + 16 (its header-protection sample would
 * leave the packet: a QUIC stack drops such packets before decryption), or for seal pn_len outside 1..4 or pn >= 2^62.
 * n == 0 makes a batch whose calls succeed and launch nothing.
 * quic_batch_records: the inner record batch, borrowed (freed with the QUIC batch): ptls_hip_batch_set_lanes,
 * _set_chacha_lanes and _set_max_workgroups work on it as on any batch. */
typedef struct st_ptls_hip_quic_batch_t ptls_hip_quic_batch_t;
ptls_hip_quic_batch_t *ptls_hip_quic_batch_new(ptls_hip_engine_t *engine, const ptls_hip_quic_packet_t *pkts, size_t n, int open,
                                               void *stream);
void ptls_hip_quic_batch_free(ptls_hip_quic_batch_t *batch);
ptls_hip_batch_t *ptls_hip_quic_batch_records(ptls_hip_quic_batch_t *batch);

/* Both calls: all buffers are device memory, the call is asynchronous on `stream`, the cipher (AES-128-GCM, AES-256-GCM or
 * ChaCha20-Poly1305) is the keyset's (ptls_hip_keyset_algo), and hp_ks must be of the same algorithm and key size, as for
 * seal_batch_supp.  PTLS_HIP_EINVAL, nothing launched, for a key or hp_key outside its keyset (the message names the
 * packet), keysets of different algorithms or key sizes, a seal batch passed to open or an open batch passed to seal, or
 * a null buffer.
 *
 * seal: the caller has written the unprotected header (pn_offset + pn_len bytes, the truncated packet number included) at
 * pkt + pkt_off.  The call seals the pkt_len - pn_offset - pn_len - 16 payload bytes at in + data_off (AAD = that header,
 * nonce from pn) into the packet right after the header, takes the 16-byte sample at pn_offset + 4 and protects the header
 * in place (RFC 9001 §5.4.1: first byte ^= mask[0] & 0x0f for a long header, & 0x1f for a short one; packet-number byte j
 * ^= mask[1 + j]).  `in` may be `pkt` itself with data_off = pkt_off + pn_offset + pn_len.  Exactly the packet's pkt_len
 * bytes change in `pkt`.
 *
 * open: unless PTLS_HIP_QUIC_UNPROTECTED is set, the mask is computed from the sample and removed from the first byte,
 * pn_len = (first & 3) + 1 is read, that many packet-number bytes are unmasked, and those 1 + pn_len bytes are written back
 * into `pkt` (nothing else in `pkt` is written: the caller can then read the key phase and the reserved bits).  With the
 * flag, pn_len is read from the first byte as it stands.  The full packet number, decoded from the truncated one and the
 * expected `pn` as in RFC 9000 Appendix A.3, goes to pn_out[i].  The record is then opened as by the open_batch calls:
 * AAD = the unprotected header, plaintext to out + data_off (written even on failure), result[i] = payload length or
 * UINT64_MAX on authentication failure.  `out` must not overlap `pkt`.  A packet that fails under one key can be
 * re-submitted under another (the next key phase) with the flag set.
 *
 * Ordering: an open call rewrites the batch's device descriptors (record length, AAD length, input offset and nonce are
 * known only once the header is unprotected), and the seal call's masks pass through a buffer of the batch.  Calls on one
 * QUIC batch must therefore be ordered: on the same stream, or by the caller's own synchronisation.
 *
 * Packets in host memory go through the host pipelines with ptls_hip_pipeline_quic_seal / _open (2g).
 * Received datagrams are split into these descriptors on the device by ptls_hip_quic_parse_datagrams (2h): coalesced
 * packets, the long-header fields up to pn_offset and pkt_len, and the key slot from the Destination Connection ID.
 * Out of scope: the node API (2d); handling Retry and Version Negotiation packets (they carry no packet protection; 2h
 * reports them and the host answers); choosing the key by key phase in these batches (the AES planner needs every packet's
 * key slot on the host; 2i plans on the device where the kernel's plan does not depend on the keys, 2j chooses the receive key
 * by Key Phase bit there, and 2l the send key, with the packet numbers and the headers). */
int ptls_hip_quic_seal_batch(ptls_hip_quic_batch_t *batch, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, const void *in,
                             void *pkt, void *stream);
int ptls_hip_quic_open_batch(ptls_hip_quic_batch_t *batch, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, void *pkt, void *out,
                             uint64_t *result, uint64_t *pn_out, void *stream);

/* ------------------------------------------------------------------------------------------ *
 * 2f. QUIC packet-protection keys, derived on the device (RFC 9001 §5.1, §5.2, §6; RFC 9369)     *
 * ------------------------------------------------------------------------------------------ */

/* The keys of the 2e batches from traffic secrets or Destination Connection IDs, for many connections per call, as picotls
 * derives them for one (ptls_hkdf_expand_label under the "tls13 quic " label prefix of ptls_aead_new, lib/picotls.c).  `ks`
 * holds the AEAD keys and static IVs, `hp_ks` the header-protection keys (zero IVs); both must belong to one engine and be
 * of one algorithm and key size.  `labels` selects the label prefix <p>: */
#define PTLS_HIP_QUIC_LABELS_V1 1 /* "quic key", "quic iv", "quic hp", "quic ku"          (RFC 9001) */
#define PTLS_HIP_QUIC_LABELS_V2 2 /* "quicv2 key", "quicv2 iv", "quicv2 hp", "quicv2 ku"  (RFC 9369) */

/* set_quic_secrets: `secrets` = count traffic secrets of hash_size bytes in host memory (32: SHA-256; 48: SHA-384, for an
 *   AES-256 keyset only; a ChaCha20-Poly1305 keyset takes 32 only).  Slot first + i of ks gets
 *   key = HKDF-Expand-Label(secret_i, "<p> key", "", key_size) and iv = HKDF-Expand-Label(secret_i, "<p> iv", "", 12); slot
 *   first + i of hp_ks gets HKDF-Expand-Label(secret_i, "<p> hp", "", key_size) with a zero IV.
 * update_quic_secrets: the key update of RFC 9001 §6.  Every secret becomes HKDF-Expand-Label(secret, "<p> ku", "",
 *   hash_size) -- written back to `secrets` -- and ks is re-keyed from the new secret.  The header-protection key does not
 *   change with a key update, so there is no hp_ks.  A receiver keeps one keyset per key phase and updates the one of the
 *   next phase; or, for the device-side choice of 2j, three banks of one keyset (slot c + stride * (generation % 3)) and
 *   updates the range of the bank the oldest generation has left.
 * set_quic_initial: the Initial keys of RFC 9001 §5.2.  `dcids` = count client Destination Connection IDs at a 20-byte
 *   stride in host memory, dcid_lens[i] = 0..20 the length of each; `salt` (1..64 bytes) is the version's initial salt,
 *   supplied by the caller: 38762cf7f55934b34d179ae6a4c80cadccbb7f0a for QUIC v1 (RFC 9001 §5.2), with labels V1;
 *   0dede3def700a6db819381be6e269dcbf9bd2ed9 for QUIC v2 (RFC 9369 §3.3.1), with labels V2.
 *   initial_i = HKDF-Extract(salt, dcid_i); the client secret HKDF-Expand-Label(initial_i, "client in", "", 32) keys slot
 *   first + 2 i and the server secret ("server in") slot first + 2 i + 1 of both keysets, by the rules of set_quic_secrets.
 *   Initial packets are AES-128-GCM with SHA-256 whatever the connection negotiates later: both keysets must be AES-GCM
 *   with key_size 16, and 2 * count slots are written from `first`.
 * The keysets serve the device-resident batches of 2e and, for packets in host memory, the pipeline calls of 2g alike.
 * All three: synchronous like ptls_hip_keyset_set_secrets (`stream` is synchronised before the return); the host IV mirror
 * (ptls_hip_keyset_get_iv) follows; secrets, initial secrets and raw keys are zeroed in device scratch memory before it is
 * released; count == 0 returns 0.  PTLS_HIP_EINVAL with a message, nothing launched and no slot changed, for a null pointer,
 * a range past either keyset, count > 2^32 - 1, a hash_size that does not go with the keyset, labels other than the two
 * above, keysets of different engines, algorithms or key sizes, a dcid_lens[i] above 20, a salt_len outside 1..64, or a
 * keyset other than AES-128-GCM in the Initial call. */
int ptls_hip_keyset_set_quic_secrets(ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, size_t first, size_t count,
                                     const void *secrets, size_t hash_size, int labels, void *stream);
int ptls_hip_keyset_update_quic_secrets(ptls_hip_keyset_t *ks, size_t first, size_t count, void *secrets, size_t hash_size,
                                        int labels, void *stream);
int ptls_hip_keyset_set_quic_initial(ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, size_t first, size_t count,
                                     const void *dcids, const uint8_t *dcid_lens, const void *salt, size_t salt_len, int labels,
                                     void *stream);

/* ------------------------------------------------------------------------------------------ *
 * 2g. QUIC packet protection from and to host memory (the pipelines of 2c over the packets of 2e) *
 * ------------------------------------------------------------------------------------------ */

/* The two calls of 2e for packets that lie in host memory (recvmmsg / sendmmsg buffers), through a pipeline of 2c: the same
 * slots, slicing, overlap and transports.  `pkts` is a HOST array of n descriptors; the descriptor, the header rules, the
 * packet-number decode, PTLS_HIP_QUIC_UNPROTECTED, h_result and h_pn_out are exactly those of ptls_hip_quic_seal_batch /
 * _open_batch, with offsets relative to the host buffers.  Synchronous like every pipeline call: on return every byte is in
 * host memory.  The pipeline may be of either algorithm (ptls_hip_pipeline_new_algo); ks and hp_ks are of that algorithm and
 * of one key size (AES-128-GCM, AES-256-GCM, ChaCha20-Poly1305), filled by ptls_hip_keyset_set or derived on the device (2f):
 * a receiver whose header-protection keys exist only in a device keyset opens its host-resident packets with this call.
 *
 * Transports as in 2c.  AUTO: MAPPED when h_pkt and h_in (seal) or h_pkt and h_out (open) are pinned or registered over
 * every byte the packets touch, COPY otherwise.  h_result and h_pn_out may be unmapped on MAPPED; they then travel through
 * the slot.  A slice holds at most slice_bytes / 64 packets on either transport.
 *
 * Exact bytes, on both transports, for pageable and pinned buffers:
 *   seal: in h_pkt exactly the pkt_len bytes of each packet change; h_in is not written; h_in == h_pkt with
 *         data_off = pkt_off + pn_offset + pn_len (in place, the way QUIC stacks build packets) is allowed.
 *   open: in h_pkt only the first byte and the pn_len packet-number bytes of each packet are written, and nothing for a
 *         packet with PTLS_HIP_QUIC_UNPROTECTED.  In h_out exactly the pkt_len - pn_offset - pn_len - 16 plaintext bytes at
 *         data_off are written, on failure too, where pn_len is what the unprotected first byte says.  h_result[i] and
 *         h_pn_out[i] are written for every i < n and nothing past them.
 * The caller cannot know pn_len before the call.  The plaintext AREAS [data_off, data_off + pkt_len - pn_offset - 17) (the
 * pn_len = 1 size) must therefore be pairwise disjoint and must not overlap any packet in h_pkt.  (The copy transport brings
 * each area back whole: up to 3 bytes at its end that the kernel does not write come back as the caller had them, read when
 * the slice is planned, like the gaps of 2c.  Do not modify them, or the headers of a seal call, during the call.)
 *
 * PTLS_HIP_EINVAL with a message (which names the packet where one is at fault), nothing launched or copied and no caller
 * byte touched: the per-packet refusals of ptls_hip_quic_batch_new; a key or hp_key outside its keyset; keysets of
 * different engines, algorithms or key sizes, or not of the pipeline's algorithm; a null pipeline or keyset, or with
 * n != 0 a null buffer; open with h_out overlapping the range of h_pkt that the packets touch (host addresses: checked
 * exactly); MAPPED forced with an unmapped buffer; a buffer mapped only in part; on COPY a packet longer than slice_bytes.
 * n == 0 returns 0. */
int ptls_hip_pipeline_quic_seal(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                const ptls_hip_quic_packet_t *pkts, size_t n, const void *h_in, void *h_pkt);
int ptls_hip_pipeline_quic_open(ptls_hip_pipeline_t *p, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                const ptls_hip_quic_packet_t *pkts, size_t n, void *h_pkt, void *h_out, uint64_t *h_result,
                                uint64_t *h_pn_out);

/* ------------------------------------------------------------------------------------------ *
 * 2h. QUIC datagrams parsed on the device: coalesced packets, long headers, connection-ID lookup  *
 *     (RFC 8999, RFC 9000 §12.2, §16, §17, RFC 9369 §3.2)                                         *
 * ------------------------------------------------------------------------------------------ */

/* The receive side in front of 2e: UDP datagrams in device memory go in, the packet descriptors of 2e come out, ready for
 * ptls_hip_quic_batch_new(..., open = 1), each with an info record.  The host still plans the open batch (40 + 32 bytes per
 * packet come back instead of the packets) and decides what to do with Retry, Version Negotiation and unknown-version
 * packets.  (The receive object of 2i keeps the entries on the device and opens them from there.) */

#define PTLS_HIP_QUIC_TYPE_INITIAL 0u
#define PTLS_HIP_QUIC_TYPE_ZERO_RTT 1u
#define PTLS_HIP_QUIC_TYPE_HANDSHAKE 2u
#define PTLS_HIP_QUIC_TYPE_RETRY 3u
#define PTLS_HIP_QUIC_TYPE_ONE_RTT 4u
#define PTLS_HIP_QUIC_TYPE_VERSION_NEGOTIATION 5u
#define PTLS_HIP_QUIC_TYPE_UNKNOWN_VERSION 6u /* a long header of a version other than 0, 1 and 0x6b3343cf */
#define PTLS_HIP_QUIC_TYPE_NONE 7u            /* a long header cut off before its version */
#define PTLS_HIP_QUIC_STATUS_OK 0u
#define PTLS_HIP_QUIC_STATUS_TRUNCATED 1u     /* a header field, the token or Length reaches past the datagram's end */
#define PTLS_HIP_QUIC_STATUS_TOO_SHORT 2u     /* less than 20 bytes behind pn_offset: no room for the header-protection sample */
#define PTLS_HIP_QUIC_STATUS_BAD_CID_LEN 3u   /* a connection-ID length above 20 under version 1 or 2 */
#define PTLS_HIP_QUIC_STATUS_BAD_FIXED_BIT 4u /* the fixed bit (0x40) is clear and require_fixed_bit is set */
#define PTLS_HIP_QUIC_INFO_MORE 1u            /* flags: the datagram holds bytes behind this, its max_per_dgram-th, entry */
#define PTLS_HIP_QUIC_NO_CONN 0xffffffffu

/* The connection-ID map: Destination Connection ID (0..20 bytes; the empty one is a valid key) -> connection number, which
 * the parse call writes into `key`, `hp_key` and `conn`.  Resident on the device as an open-addressing table of 32-byte
 * entries with linear probing, sized to the next power of two >= 2 * capacity (load <= 0.5); the host keeps the
 * authoritative mirror, removes with a backward shift (no tombstones) and uploads what changed.  The device only reads it.
 * cids = count connection IDs at a 20-byte stride in host memory, cid_lens[i] = 0..20, as in 2f.
 * set inserts or replaces; remove of an absent CID is not an error.  Both are synchronous like
 * ptls_hip_keyset_set_quic_secrets and must not run concurrently with each other or with a parse call on the same map.
 * PTLS_HIP_EINVAL with a message and nothing changed for a null pointer (cids / cid_lens / conns with count != 0), a
 * cid_lens[i] above 20, a conns[i] of PTLS_HIP_QUIC_NO_CONN, or a set after which the map would hold more than `capacity`
 * CIDs; cidmap_new: NULL for a null engine or a capacity outside 1 .. 2^30.  cidmap_free waits for the parse calls that
 * used the map. */
typedef struct st_ptls_hip_quic_cidmap_t ptls_hip_quic_cidmap_t;
ptls_hip_quic_cidmap_t *ptls_hip_quic_cidmap_new(ptls_hip_engine_t *engine, size_t capacity);
void ptls_hip_quic_cidmap_free(ptls_hip_quic_cidmap_t *map);
size_t ptls_hip_quic_cidmap_size(ptls_hip_quic_cidmap_t *map); /* CIDs in the map */
int ptls_hip_quic_cidmap_set(ptls_hip_quic_cidmap_t *map, size_t count, const void *cids, const uint8_t *cid_lens,
                             const uint32_t *conns, void *stream);
int ptls_hip_quic_cidmap_remove(ptls_hip_quic_cidmap_t *map, size_t count, const void *cids, const uint8_t *cid_lens,
                                void *stream);

typedef struct st_ptls_hip_quic_datagram_t { /* 16 bytes */
    uint64_t off;      /* first byte of the datagram in d_buf */
    uint32_t len;      /* <= 65535; 0 = no entry */
    uint32_t reserved;
} ptls_hip_quic_datagram_t;

typedef struct st_ptls_hip_quic_pktinfo_t { /* 32 bytes; entry k describes packet descriptor k */
    uint32_t dgram;     /* index of the datagram the packet came in */
    uint32_t version;   /* long headers; 0 for a short header */
    uint32_t conn;      /* the map's value for the DCID, or PTLS_HIP_QUIC_NO_CONN */
    uint32_t token_len; /* Initial */
    uint16_t dcid_off, scid_off, token_off; /* from the packet's first byte; 0 = the field was not reached or does not exist */
    uint8_t dcid_len, scid_len;
    uint8_t type;       /* PTLS_HIP_QUIC_TYPE_* */
    uint8_t status;     /* PTLS_HIP_QUIC_STATUS_* */
    uint8_t flags;      /* PTLS_HIP_QUIC_INFO_MORE */
    uint8_t pad[5];     /* 0 */
} ptls_hip_quic_pktinfo_t;

typedef struct st_ptls_hip_quic_parse_params_t {
    uint32_t short_cid_len;        /* 0..20: the length of the DCIDs this endpoint issued (short headers do not carry it) */
    uint32_t max_per_dgram;        /* 1..16: entries per datagram */
    uint32_t require_fixed_bit;    /* != 0: a clear fixed bit is an error; 0: the bit is not looked at (RFC 9287) */
    uint32_t reserved;             /* 0 */
    const uint64_t *d_expected_pn; /* device: expected packet number of connection c, space s at [3 c + s], or NULL */
    size_t expected_count;         /* entries of d_expected_pn */
} ptls_hip_quic_parse_params_t;

/* Walks the n datagrams dgrams[i] (a HOST array) in the device buffer d_buf (buf_len bytes) and writes one
 * ptls_hip_quic_packet_t and one ptls_hip_quic_pktinfo_t per entry into the HOST arrays h_pkts and h_info (cap entries each).
 * Synchronous: on return `stream` has been synchronised and the entries are in the host arrays.  Entries are dense, in
 * datagram order and within a datagram in wire order; the same input gives the same bytes; exactly *n_pkts entries are
 * written and nothing past them.  No byte at or past a datagram's end is read.
 *
 * The walk of one packet, with `rest` = the bytes from its first byte to the datagram's end:
 *   short header (first & 0x80 == 0): type ONE_RTT; dcid_off 1, dcid_len short_cid_len, pn_offset = 1 + short_cid_len; the
 *     packet takes the rest of the datagram (RFC 9000 §12.2); rest < pn_offset + 20 is TOO_SHORT.
 *   long header: version (big-endian at 1), DCID length at 5, the DCID, the SCID length, the SCID; a field past the
 *     datagram's end is TRUNCATED.  Version 0 is VERSION_NEGOTIATION, a version other than 1 and 0x6b3343cf is
 *     UNKNOWN_VERSION: both take the rest of the datagram, with DCID and SCID (up to 255 bytes) by the invariants of RFC 8999.
 *     Version 1 has the type bits Initial 0, 0-RTT 1, Handshake 2, Retry 3; version 0x6b3343cf those of RFC 9369 §3.2: Retry
 *     0, Initial 1, 0-RTT 2, Handshake 3.  Under these two a CID length above 20 is BAD_CID_LEN; Retry takes the rest of the
 *     datagram; Initial carries the token-length varint and the token; Initial, 0-RTT and Handshake carry the Length varint
 *     (any of the four widths, non-minimal encodings included), pn_offset is the first byte behind it and
 *     pkt_len = pn_offset + Length; Length < 20 is TOO_SHORT, pn_offset + Length > rest is TRUNCATED.
 *   With require_fixed_bit, a short packet or a long one of version 1 or 0x6b3343cf with first & 0x40 == 0 is BAD_FIXED_BIT
 *     (checked before the lengths).
 *   Every status but OK ends the datagram: the entry covers the rest of it, with pn_offset 0; the info fields reached before
 *   the error stand, the others are 0.  Retry, Version Negotiation and unknown-version entries have status OK and pn_offset 0.
 *   An entry is openable if and only if pn_offset != 0; then pkt_len >= pn_offset + 20, so ptls_hip_quic_batch_new takes it.
 * A zero-length datagram gives no entry.  A datagram with more than max_per_dgram entries: its last entry carries
 * PTLS_HIP_QUIC_INFO_MORE and the rest is dropped.  The RFC 9000 §12.2 rule that later coalesced packets with another DCID
 * are ignored is the host's: it sees the conn of each entry.
 *
 * Each packet descriptor: pkt_off = the absolute offset in d_buf; pkt_len, pn_offset from the walk;
 * data_off = pkt_off + pn_offset + 1 (with the open call's `out` a separate buffer of d_buf's size, the plaintext areas are
 * pairwise disjoint by construction); pn_len = 0, flags = 0; key = hp_key = conn = the map's value for the DCID
 * (status OK and dcid_len <= 20) or PTLS_HIP_QUIC_NO_CONN (no match, or map == NULL), which the open call refuses by name as
 * a key slot outside the keyset; pn = d_expected_pn[3 conn + space] with space 0 for Initial, 1 for Handshake, 2 for 0-RTT and
 * 1-RTT, when the entry is openable, the table is not NULL, a connection matched and the index is below expected_count,
 * else 0.
 *
 * PTLS_HIP_EINVAL with a message, nothing launched and nothing written (except *n_pkts where stated): a null engine,
 * params or n_pkts, or with n != 0 a null dgrams or d_buf, or with cap != 0 a null h_pkts or h_info; n > 2^32 - 1 or
 * n * max_per_dgram > 2^32 - 1; a datagram with len > 65535 or off + len > buf_len (the message names its index);
 * short_cid_len above 20, max_per_dgram outside 1..16 or reserved != 0; a map of another engine.  cap smaller than the
 * number of entries: PTLS_HIP_EINVAL after the counting pass, *n_pkts = the number needed, the host arrays untouched (cap = 0
 * is the sizing call).  n == 0 returns 0 with *n_pkts = 0. */
int ptls_hip_quic_parse_datagrams(ptls_hip_engine_t *engine, const ptls_hip_quic_parse_params_t *params,
                                  ptls_hip_quic_cidmap_t *map, const ptls_hip_quic_datagram_t *dgrams, size_t n,
                                  const void *d_buf, size_t buf_len, ptls_hip_quic_packet_t *h_pkts,
                                  ptls_hip_quic_pktinfo_t *h_info, size_t cap, size_t *n_pkts, void *stream);
/* Diagnostic (tools/bench_quic_parse.py): enable != 0 makes the calling thread's parse calls time themselves with HIP events;
 * kernels_ms / d2h_ms (either may be NULL) receive the last such call's kernel time (upload of the datagram array, count,
 * scan and write passes) and the time of the copies of the entries back to the host. */
void ptls_hip_quic_parse_timing(int enable, float *kernels_ms, float *d2h_ms);

/* ------------------------------------------------------------------------------------------ *
 * 2i. the receive object: parsed entries stay on the device and are selected, packed, planned   *
 *     and opened from there                                                                     *
 * ------------------------------------------------------------------------------------------ */

/* 2h followed by 2e costs a copy of 72 bytes per packet to the host, the host's planning of the open batch and the upload of
 * its plan.  A receive object keeps the entries of a parse call in device memory and opens them with one call: which entries
 * can be opened is decided on the device, they are packed in entry order, the planner's sums are taken there, and for the
 * ChaCha20-Poly1305 kernel (which needs no plan) and the wave-per-record AES kernel (whose plan is a sort by length) the
 * existing header and record kernels follow at once.  The host reads five 64-bit sums per open call.  Where the planner wants
 * the AES batch kernel (key runs of 20 records and more on average), the packed descriptors (40 bytes each) go back to the
 * host and through ptls_hip_quic_batch_new / ptls_hip_quic_open_batch unchanged (report.planned_on_device = 0).
 *
 * rx_new: room for max_dgrams datagrams per parse call and cap entries; device memory is allocated with the first use of each
 *   array and kept, so the calls allocate nothing per call.  NULL for a null engine, cap outside 1 .. 2^32 - 1 or max_dgrams
 *   above 2^32 - 1.  rx_free waits for the launches that used the object.
 * rx_parse: the walk, the rules and the refusals of ptls_hip_quic_parse_datagrams, byte for byte, into the object's device
 *   arrays; the host learns *n_pkts only.  Also PTLS_HIP_EINVAL: n above max_dgrams; more entries than cap (after the
 *   counting pass, *n_pkts = the number needed, no entry loaded).  Synchronises `stream` once (the count).
 * rx_set_packets: instead, n descriptors, and optionally their info records, that the caller already has in DEVICE memory
 *   (copied on `stream`); PTLS_HIP_EINVAL for n above cap.  Either call replaces the entries loaded before; n == 0 unloads.
 * rx_packets / rx_info / rx_count: the loaded entries (device pointers, NULL when none / no info records) and their number.
 *
 * rx_open selects entry k if and only if
 *   pn_offset != 0, pn_offset + 20 <= pkt_len <= 65535, pkt_off + pkt_len <= buf_len,
 *   data_off + (pkt_len - pn_offset - 17) <= out_len   (the plaintext area at its pn_len = 1 size),
 *   key < the slots of ks and hp_key < the slots of hp_ks   (PTLS_HIP_QUIC_NO_CONN never is),
 *   and, where info records are loaded, (type_mask >> info[k].type) & 1.
 * These are the per-packet refusals of 2e's calls, applied per packet on the device: an unselected entry is skipped, not an
 * error.  Selected entries keep their order: d_sel[j] = the entry index of the j-th selected packet, d_result[j] and
 * d_pn_out[j] as ptls_hip_quic_open_batch defines them for it; exactly report->n_selected elements of each are written.  In
 * d_buf only the 1 + pn_len header bytes of selected packets are written (none with PTLS_HIP_QUIC_UNPROTECTED in the
 * descriptor's flags), in d_out exactly their plaintext bytes, on failure too.  One parse may be followed by several opens
 * with other masks and keysets (Handshake, then 1-RTT), each with its own output arrays.  All five arrays are device memory
 * (cap elements are always enough).  report->lanes: the lanes per record of the launch (64: the wave-per-record AES kernel).
 * PTLS_HIP_EINVAL, nothing launched: a null object, keyset or report; keysets of another engine than the object's, or of
 * different algorithms or key sizes; with entries loaded, a null buffer or [d_buf, buf_len) overlapping [d_out, out_len).
 * No entries loaded: 0 with n_selected = 0.
 * Ordering: calls on one receive object must be ordered by the caller (same stream, or own synchronisation), as for a QUIC
 * batch.  rx_open synchronises `stream` once, to read the sums, and returns with the header and record kernels in flight;
 * on the host-planned path it returns when they are done.
 *
 * rx_set_plan: 0 = as above; 1 = the device plan whatever the key runs (AES: the wave-per-record kernel); 2 = the host plan
 *   for every cipher.  For tests and A/B measurements: the outputs are the same.  PTLS_HIP_EINVAL for another value.
 * rx_order: device array of n_selected positions, the plan order of the last open call if it planned AES on the device (a
 *   stable order of the selected packets by decreasing (pkt_len - pn_offset - 17) >> 4), else NULL.
 * rx_timing: diagnostic (tools/bench_quic_rx.py), as ptls_hip_quic_parse_timing: HIP-event times of the last rx_open's
 *   select / scan / compact / sums launches and of its sort launches.
 * Out of scope: key-run chunks for the AES batch kernel made on the device; grouping interleaved packets by key; key slots
 * for Initial packets of unknown connections; the host pipelines (2g) and the node API (2d).  The key phase: rx_open takes
 * `key` as it is; rx_open_keyphase (2j) chooses the generation on the device. */
typedef struct st_ptls_hip_quic_rx_t ptls_hip_quic_rx_t;
typedef struct st_ptls_hip_quic_rx_report_t {
    uint64_t n_selected;
    int32_t planned_on_device;
    int32_t lanes;
} ptls_hip_quic_rx_report_t;
ptls_hip_quic_rx_t *ptls_hip_quic_rx_new(ptls_hip_engine_t *engine, size_t max_dgrams, size_t cap);
void ptls_hip_quic_rx_free(ptls_hip_quic_rx_t *rx);
int ptls_hip_quic_rx_parse(ptls_hip_quic_rx_t *rx, const ptls_hip_quic_parse_params_t *params, ptls_hip_quic_cidmap_t *map,
                           const ptls_hip_quic_datagram_t *dgrams, size_t n, const void *d_buf, size_t buf_len, size_t *n_pkts,
                           void *stream);
int ptls_hip_quic_rx_set_packets(ptls_hip_quic_rx_t *rx, const ptls_hip_quic_packet_t *d_pkts,
                                 const ptls_hip_quic_pktinfo_t *d_info, size_t n, void *stream);
const ptls_hip_quic_packet_t *ptls_hip_quic_rx_packets(ptls_hip_quic_rx_t *rx);
const ptls_hip_quic_pktinfo_t *ptls_hip_quic_rx_info(ptls_hip_quic_rx_t *rx);
size_t ptls_hip_quic_rx_count(ptls_hip_quic_rx_t *rx);
int ptls_hip_quic_rx_open(ptls_hip_quic_rx_t *rx, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, uint32_t type_mask, void *d_buf,
                          size_t buf_len, void *d_out, size_t out_len, uint32_t *d_sel, uint64_t *d_result, uint64_t *d_pn_out,
                          ptls_hip_quic_rx_report_t *report, void *stream);
int ptls_hip_quic_rx_set_plan(ptls_hip_quic_rx_t *rx, int mode);
const uint32_t *ptls_hip_quic_rx_order(ptls_hip_quic_rx_t *rx);
void ptls_hip_quic_rx_timing(int enable, float *select_ms, float *plan_ms);

/* ------------------------------------------------------------------------------------------ *
 * 2j. receive keys chosen by Key Phase bit on the device, and key updates committed there        *
 *     (RFC 9001 §6)                                                                              *
 * ------------------------------------------------------------------------------------------ */

/* The Key Phase bit (0x04 of a short header's first byte) sits under header protection, and with 2f the header-protection
 * keys exist only in a device keyset: the host cannot see the bit.  rx_open_keyphase is rx_open with the AEAD key slot of
 * every short-header packet chosen by the header kernel from that bit and a small per-connection state in device memory;
 * rx_keyphase_commit moves that state on from the authenticated results, so that the next call chooses correctly without
 * the host having looked at a packet.
 *
 * The state is a caller-owned DEVICE array of 16-byte entries, indexed by the connection number that the parse call writes
 * into `key`.  The keys of generation g of connection c live in slot c + stride * (g % 3) of ONE AEAD keyset with at least
 * 3 * stride slots: three banks hold the previous, the current and the next generation, and the keys of generation g + 2
 * overwrite those of g - 1 (RFC 9001 §6.5).  The header-protection key does not change with a key update: hp_ks and hp_key
 * are used as they are. */
typedef struct st_ptls_hip_quic_keyphase_t {
    uint64_t first_pn; /* lowest packet number opened under the current generation; UINT64_MAX: none yet */
    uint32_t gen;      /* generation of the current receive keys (<= 2^32 - 2); its Key Phase bit is gen & 1 */
    uint32_t reserved; /* 0 */
} ptls_hip_quic_keyphase_t;
#define PTLS_HIP_QUIC_NO_GEN 0xffffffffu

/* rx_open_keyphase: for a short-header packet, with `bit` the unmasked Key Phase bit (with PTLS_HIP_QUIC_UNPROTECTED: the bit
 *   of the first byte as it stands) and pn the decoded full packet number,
 *       g' = gen        if bit == (gen & 1)
 *          = gen - 1    else if gen > 0 and pn < first_pn    (a reordered packet from before the update)
 *          = gen + 1    otherwise                            (the peer has updated)
 *   and the packet is opened under slot key + stride * (g' % 3); d_gen_out[j] = g'.  first_pn == UINT64_MAX makes every
 *   packet with the other bit a previous-generation packet (right after a locally initiated update, before the peer has
 *   answered); gen == 0 has no previous generation.  A long-header packet (0x80 set) is opened under slot `key` itself and
 *   gets d_gen_out[j] = PTLS_HIP_QUIC_NO_GEN, whatever its low bits are.  Exactly one key is tried per packet: a packet sealed
 *   under any other generation fails (UINT64_MAX), with d_gen_out[j] still the rule's value.
 *   Everything else is rx_open's, with one change to the select rule: key < min(stride, count) takes the place of key < the
 *   slots of ks.  d_gen_out is device memory like d_result: exactly report->n_selected elements are written.
 *   The plan: ChaCha20-Poly1305 as in rx_open.  AES always takes the wave-per-record kernel (planned_on_device = 1,
 *   lanes = 64), whatever the key runs say: the batch kernel's key-run chunks cannot carry a per-record key.  For bulk traffic
 *   of one connection that is the slower record kernel: 262 144 packets of 1 350 bytes on one key take it 1.6 ms, the batch
 *   kernel about 0.45 ms.  A receiver that wants the batch kernel's rate for such traffic uses rx_open with
 *   the generation it knows.
 *   PTLS_HIP_EINVAL, nothing launched, besides rx_open's refusals: a null kp, d_phase or d_gen_out; stride == 0 or
 *   count == 0; 3 * stride above the slots of ks; rx_set_plan mode 2 (the host plan fixes a chunk's key on the host).
 *   ks and hp_ks are in use until the launches are done, as for rx_open; the state array is read by the header kernel.
 * rx_keyphase_commit: follows the rx_open_keyphase whose d_result, d_pn_out and d_gen_out it is given, on the same stream,
 *   before the next open on the object (it reads the connection of selected packet j from the object's packed descriptors).
 *   For every connection c < count, let N be its selected packets with d_result != UINT64_MAX and d_gen_out == gen + 1, and C
 *   those with d_gen_out == gen.  N not empty: gen += 1, first_pn = min pn over N, and c is listed in d_updated.  Otherwise,
 *   C not empty: first_pn = min(first_pn, min pn over C).  Otherwise the entry is unchanged.  Packets that failed
 *   authentication, previous-generation packets and long-header packets change nothing: a forged packet with a flipped bit
 *   does not advance a connection (RFC 9001 §6.3).  d_updated (device, room for `count` elements) receives the updated
 *   connections in ascending order, *n_updated their number: the host then derives the keys of generation gen + 1 of exactly
 *   those connections into the bank that generation gen - 2 has left (ptls_hip_keyset_update_quic_secrets).  It never reads a
 *   result array.  The outcome does not depend on the order in which the packets are looked at.  One stream
 *   synchronisation, to read the count.
 *   PTLS_HIP_EINVAL, nothing launched: a null pointer; count == 0 or above 2^32 - 1; no rx_open_keyphase on the object since
 *   its entries were loaded or since a plain rx_open.
 * Out of scope: the key phase with the AES batch kernel (key-run chunks made on the device), with the QUIC batches of 2e and
 * the host pipelines of 2g (the send side follows a committed update in 2l); an indexed update_quic_secrets (today: contiguous ranges); checking the reserved bits; the usage limits of RFC 9001 §6.6 and the handshake-confirmed rule of §6.2. */
typedef struct st_ptls_hip_quic_rx_keyphase_t {
    const ptls_hip_quic_keyphase_t *d_phase; /* device: the per-connection state */
    size_t count;                            /* its entries */
    size_t stride;                           /* the bank stride in ks */
    uint32_t *d_gen_out;                     /* device: one generation per selected packet, like d_result */
} ptls_hip_quic_rx_keyphase_t;
int ptls_hip_quic_rx_open_keyphase(ptls_hip_quic_rx_t *rx, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, uint32_t type_mask,
                                   const ptls_hip_quic_rx_keyphase_t *kp, void *d_buf, size_t buf_len, void *d_out,
                                   size_t out_len, uint32_t *d_sel, uint64_t *d_result, uint64_t *d_pn_out,
                                   ptls_hip_quic_rx_report_t *report, void *stream);
int ptls_hip_quic_rx_keyphase_commit(ptls_hip_quic_rx_t *rx, ptls_hip_quic_keyphase_t *d_phase, size_t count,
                                     const uint64_t *d_result, const uint64_t *d_pn_out, const uint32_t *d_gen_out,
                                     uint32_t *d_updated, size_t *n_updated, void *stream);
/* Diagnostic (tools/bench_quic_keyphase.py): with ptls_hip_quic_rx_timing enabled on the calling thread, the HIP-event times of
 * the last rx_open_keyphase's header kernel and of the last rx_keyphase_commit's launches (either pointer may be NULL). */
void ptls_hip_quic_rx_keyphase_timing(float *header_ms, float *commit_ms);

/* ------------------------------------------------------------------------------------------ *
 * 2k. received packet numbers tracked on the device: replays, and the expected packet number     *
 *     (RFC 9000 §12.3, §13.2.3, §17.1)                                                           *
 * ------------------------------------------------------------------------------------------ */

/* The parse call decodes a truncated packet number against d_expected_pn[3 c + s], and a receiver must discard a packet
 * unless it is certain that it has not processed one with the same number in that space (RFC 9000 §12.3).  rx_track settles
 * both from the authenticated results of an open call, on the device: it keeps, per connection and packet-number space, the
 * largest number accepted and a 64-packet window of accepted numbers, gives every selected packet a verdict, advances the
 * table that the next parse call reads, and lists the connections that received something new.  The host reads one count and
 * never a result array.  Like the key-phase commit, forged packets change nothing.
 *
 * The state is a caller-owned DEVICE array of 16-byte entries; entry [3 c + s] is for connection c (the value the parse call
 * writes into `key`) and space s: Initial 0, Handshake 1, 0-RTT and 1-RTT 2. */
typedef struct st_ptls_hip_quic_pnspace_t {
    uint64_t next;   /* largest accepted packet number + 1; 0: none yet */
    uint64_t window; /* bit k (k < 64): packet number next - 1 - k has been accepted; 0 when next == 0 */
} ptls_hip_quic_pnspace_t;
#define PTLS_HIP_QUIC_PN_NONE 0u      /* failed authentication, or not tracked: changes nothing */
#define PTLS_HIP_QUIC_PN_NEW 1u
#define PTLS_HIP_QUIC_PN_DUPLICATE 2u
#define PTLS_HIP_QUIC_PN_TOO_OLD 3u   /* more than 64 behind the largest: cannot be proven new, discard */

/* rx_track: follows an rx_open or rx_open_keyphase on the same stream, with that call's d_sel, d_result and d_pn_out, before
 *   the next open or load on the object (it reads the connection of selected packet j from the object's packed descriptors
 *   and its type from the object's info records through d_sel).  It may come before or after rx_keyphase_commit: neither reads
 *   what the other writes.
 *   Selected packet j is tracked if d_result[j] != UINT64_MAX, its connection is below `count` and its type is Initial,
 *   0-RTT, Handshake or 1-RTT.  Every other packet gets PN_NONE and touches no state: a forged packet with a huge decoded
 *   number advances nothing.  A tracked packet with pn = d_pn_out[j], in a space whose state BEFORE the call is (next, window):
 *     1. pn < next and next - 1 - pn >= 64: PN_TOO_OLD.
 *     2. pn < next and bit next - 1 - pn of window set: PN_DUPLICATE.
 *     3. otherwise, a tracked packet j' < j of the same space has the same pn: PN_DUPLICATE (the lowest position wins).
 *     4. otherwise PN_NEW.
 *   Rule 1 looks at the state before the call: a bulk batch of fresh packets of one connection is all PN_NEW.
 *   After the call, next' = max(next, 1 + the largest pn among the NEW packets) and window' = window << (next' - next) (0 for
 *   a shift of 64 or more) OR bit next' - 1 - pn of every NEW packet with next' - 1 - pn < 64.  NEW packets further back are
 *   accepted and not remembered: a later replay of one is PN_TOO_OLD, so nothing behind the window is accepted twice.  A space
 *   without a NEW packet keeps its 16 bytes.  The outcome does not depend on the order in which the packets are looked at.
 *   Exactly n_selected elements of d_verdict are written.  d_expected_pn[3 c + s] = next' is written for every space with a
 *   NEW packet and 3 c + s < expected_count, and no other element.  d_touched receives the connections with at least one NEW
 *   packet in ascending order, *n_touched their number; exactly that many elements are written.  One stream
 *   synchronisation, to read the count.  Nothing selected: 0 with *n_touched = 0 and nothing written.
 *   PTLS_HIP_EINVAL, nothing launched: a null object, struct, d_spaces, d_verdict, d_touched, d_sel, d_result, d_pn_out or
 *   n_touched; count == 0 or above 2^32 - 1; d_expected_pn == NULL with expected_count != 0; no open on the object since its
 *   entries were loaded; entries loaded without info records (rx_set_packets with d_info == NULL).
 *   The call's scratch belongs to the object: allocated with the first use, grown when a call needs more, released by rx_free.
 * ACK frames and ACK ranges for the listed connections: 2m, from d_touched as it is.
 * Out of scope: windows wider than 64; the batches of 2e, the pipelines of 2g and the node API; discarding packet-number
 * spaces; ECN counts; knowing whether a packet was ack-eliciting (a frame walk over the opened payloads). */
typedef struct st_ptls_hip_quic_rx_track_t {
    ptls_hip_quic_pnspace_t *d_spaces; /* device: 3 * count entries */
    size_t count;                      /* connections */
    uint64_t *d_expected_pn;           /* device, or NULL: the table the parse call reads */
    size_t expected_count;             /* its entries */
    uint32_t *d_verdict;               /* device: one per selected packet, like d_result */
    uint32_t *d_touched;               /* device, room for count: connections with at least one NEW packet, ascending */
} ptls_hip_quic_rx_track_t;
int ptls_hip_quic_rx_track(ptls_hip_quic_rx_t *rx, const ptls_hip_quic_rx_track_t *tr, const uint32_t *d_sel,
                           const uint64_t *d_result, const uint64_t *d_pn_out, size_t *n_touched, void *stream);
/* Diagnostic (tools/bench_quic_track.py): with ptls_hip_quic_rx_timing enabled on the calling thread, the HIP-event time of the
 * last rx_track's launches (the pointer may be NULL). */
void ptls_hip_quic_rx_track_timing(float *track_ms);

/* ------------------------------------------------------------------------------------------ *
 * 2l. the send object: packet numbers assigned, headers written and send keys chosen on the     *
 *     device (RFC 9000 §12.3, §17.1, §17.3.1, A.2; RFC 9001 §6.2)                                 *
 * ------------------------------------------------------------------------------------------ */

/* The mirror of the receive object for short-header (1-RTT) packets.  With 2e the host chooses every packet number and its
 * encoded length, writes the header bytes, knows the current key generation, fills and uploads a 40-byte descriptor per packet
 * and plans on the host.  Here the host hands over "connection c, payload at this offset, this many bytes, put the packet
 * there" as a DEVICE array of requests, and the device does the rest from a per-connection state table that it keeps up to
 * date: a call reads one count and two sums back.
 *
 * Both arrays are caller-owned DEVICE memory; entry c of the state table is connection c. */
typedef struct st_ptls_hip_quic_txconn_t { /* 48 bytes */
    uint64_t next_pn;        /* the next packet number to assign */
    uint64_t largest_acked;  /* largest packet number the peer has acknowledged; UINT64_MAX: none yet */
    uint32_t gen;            /* generation of the send keys (<= 2^32 - 2); Key Phase bit = gen & 1 */
    uint8_t dcid_len;        /* 0..20 */
    uint8_t flags;           /* bit 0: the spin bit to send; other bits 0 */
    uint8_t reserved[2];
    uint8_t dcid[20];
    uint8_t reserved2[4];
} ptls_hip_quic_txconn_t;
typedef struct st_ptls_hip_quic_txreq_t { /* 24 bytes */
    uint64_t data_off;  /* the plaintext payload in d_in */
    uint64_t pkt_off;   /* where the packet's first byte goes in d_pkt */
    uint32_t conn;
    uint32_t len;       /* payload bytes */
} ptls_hip_quic_txreq_t;
#define PTLS_HIP_QUIC_TX_SENT 0u
#define PTLS_HIP_QUIC_TX_NO_CONN 1u /* conn outside the state table, the key banks or the header-protection keyset */
#define PTLS_HIP_QUIC_TX_SPLIT 2u   /* a later run of a connection whose first run the call numbered */
#define PTLS_HIP_QUIC_TX_PN 3u      /* no packet number or no encodable length for it */
#define PTLS_HIP_QUIC_TX_RANGE 4u   /* the connection ID, the packet or the payload does not fit */

/* Keys are laid out as in 2j: the AEAD keys of generation g of connection c sit in slot c + stride * (g % 3) of ks, the
 * header-protection key in slot c of hp_ks; the host derives each next generation's send keys ahead of time into the free
 * bank, as for receive.  With d_rx_phase (2j's state array, `count` entries) the generation used for connection c is
 * max(txconn.gen, d_rx_phase[c].gen), and that value is stored back into txconn.gen: the sender follows a peer's key update
 * that rx_keyphase_commit committed (RFC 9001 §6.2) with no host step.
 *
 * The rule, over the n requests of a call; every value of the state table is the one BEFORE the call:
 *   1. A run is a maximal stretch of consecutive requests with the same conn.  A connection's packets in one call must form
 *      one run: its first run by position is numbered, every later run of it gets TX_SPLIT and touches nothing.
 *   2. TX_NO_CONN if conn >= min(count, stride, slots of hp_ks).
 *   3. Request j of a numbered run that starts at position h gets pn = next_pn + (j - h) (the sum saturates at 2^64 - 1).
 *      Requests refused under 4 and 5 still consume their number: gaps are legal (RFC 9000 §12.3).
 *   4. TX_PN if pn >= 2^62, or largest_acked != UINT64_MAX and largest_acked >= pn, or no allowed length suffices: with
 *      num_unacked = largest_acked == UINT64_MAX ? pn + 1 : pn - largest_acked, pn_len is the smallest L in
 *      max(1, params.pn_len) .. 4 with num_unacked < 2^(8 L - 1) (RFC 9000 §17.1: more than twice the range; A.2).
 *   5. TX_RANGE for dcid_len > 20, pn_len + len < 4 (the header-protection sample would leave the packet),
 *      pkt_len = 1 + dcid_len + pn_len + len + 16 > 65535, data_off + len > in_len, or pkt_off + pkt_len > buf_len; none of
 *      these sums wraps.
 *   6. Otherwise TX_SENT: the header 0x40 | spin << 5 | (gen & 1) << 2 | (pn_len - 1), the DCID, the low pn_len bytes of pn
 *      big-endian is written at d_pkt + pkt_off, and the packet is sealed under slot conn + stride * (gen % 3) and
 *      header-protected exactly as ptls_hip_quic_seal_batch would for that header.
 *   The precedence is NO_CONN, SPLIT, PN, RANGE.
 * After the call, for every connection with a numbered run: next_pn += the run's length (saturating), gen = the generation
 * used; every other byte of the table is unchanged.  d_status[j]; d_pn_out[j] = the number, or UINT64_MAX for NO_CONN and
 * SPLIT; d_pkt_len[j] = 0 unless SENT: exactly n elements of each are written.  In d_pkt exactly the pkt_len bytes of sent
 * packets change; d_in is not written.  Packet areas must be pairwise disjoint (the caller's duty, as in 2e).  The outcome does
 * not depend on the order in which the requests are looked at.
 *
 * tx_new: room for cap requests per call; the scratch is the object's, allocated with the first use of each array and kept:
 *   a steady-state call allocates nothing.  NULL for a null engine or cap outside 1 .. 2^32 - 1.  tx_free waits for the
 *   launches that used the object.
 * tx_seal: report->n_sent, ->bytes (the sum of pkt_len) and ->lanes (the lanes per record of the launch).  It synchronises
 *   `stream` once, to read its sums, and returns with the record and header kernels in flight.  n == 0 returns 0.
 *   ChaCha20-Poly1305 goes on its kernel with lanes from the sums.  AES always takes the wave-per-record kernel (lanes = 64)
 *   behind a stable sort by block count, as rx_open_keyphase does and for 2j's reason: the batch kernel's key-run chunks, planned
 *   on the host, cannot carry a per-record key.  2j measured that kernel at 1.6 ms against the batch kernel's 0.45 ms for 262 144
 *   packets of 1 350 bytes on one key; that is the known price here for bulk traffic of one connection, and a sender that wants
 *   the batch kernel's rate for such traffic uses 2e.  On the send side that batch measured 2.0 ms for this call against 0.5 ms for a planned
 *   2e batch's seal, and 9.9 ms for the 2e path with its host steps.
 *   PTLS_HIP_EINVAL, nothing launched and no byte touched: a null object, keyset, params, report, state, output array, or with
 *   n != 0 a null request array or buffer; n above cap; count == 0 or above 2^32 - 1; stride == 0; 3 * stride above the slots
 *   of ks; pn_len above 4 or a non-zero params.reserved; keysets of another engine than the object's, or of different algorithms or key sizes;
 *   [d_in, in_len) overlapping [d_pkt, buf_len).
 *   Ordering: calls on one send object, and calls that write its state table, must be ordered by the caller (same stream).
 * tx_packets / tx_count: the packed 40-byte descriptors (2e's) of the last call's sent packets, in request order (a device
 *   pointer, NULL when none), and their number.
 * tx_timing: diagnostic (tools/bench_quic_tx.py), as rx_timing: with it enabled on the calling thread, the HIP-event times of
 *   the last tx_seal's launches in front of the record kernel (numbering, select, build, state) and of its sort launches.
 * ACK frames and their requests come from 2m (rx_ack writes d_reqs on the device).
 * Out of scope: long headers; coalescing; padding; building other frames, and bundling them with an ACK frame; reading
 * received ACK frames into largest_acked; in-place payloads (d_in inside d_pkt); the host pipelines
 * (2g) and the node API (2d); the AEAD usage limits of RFC 9001 §6.6; the host plan (key-run chunks for the AES batch
 * kernel). */
typedef struct st_ptls_hip_quic_tx_t ptls_hip_quic_tx_t;
typedef struct st_ptls_hip_quic_tx_params_t {
    ptls_hip_quic_txconn_t *d_conns;           /* device: the per-connection send state */
    size_t count;                              /* its entries */
    size_t stride;                             /* the bank stride in ks */
    const ptls_hip_quic_keyphase_t *d_rx_phase; /* device, or NULL: 2j's receive state, `count` entries */
    uint32_t pn_len;                           /* 0: minimal; 1..4: at least that many packet-number bytes */
    uint32_t reserved;                         /* 0 */
    uint32_t *d_status;                        /* device: one PTLS_HIP_QUIC_TX_* per request */
    uint64_t *d_pn_out;                        /* device: one per request */
    uint32_t *d_pkt_len;                       /* device: one per request */
} ptls_hip_quic_tx_params_t;
typedef struct st_ptls_hip_quic_tx_report_t {
    uint64_t n_sent;
    uint64_t bytes;
    int32_t lanes;
    int32_t reserved;
} ptls_hip_quic_tx_report_t;
ptls_hip_quic_tx_t *ptls_hip_quic_tx_new(ptls_hip_engine_t *engine, size_t cap);
void ptls_hip_quic_tx_free(ptls_hip_quic_tx_t *tx);
int ptls_hip_quic_tx_seal(ptls_hip_quic_tx_t *tx, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                          const ptls_hip_quic_tx_params_t *params, const ptls_hip_quic_txreq_t *d_reqs, size_t n, const void *d_in,
                          size_t in_len, void *d_pkt, size_t buf_len, ptls_hip_quic_tx_report_t *report, void *stream);
const ptls_hip_quic_packet_t *ptls_hip_quic_tx_packets(ptls_hip_quic_tx_t *tx);
size_t ptls_hip_quic_tx_count(ptls_hip_quic_tx_t *tx);
void ptls_hip_quic_tx_timing(int enable, float *front_ms, float *sort_ms);

/* ------------------------------------------------------------------------------------------ *
 * 2m. ACK frames written on the device from the tracked packet numbers, with the send requests  *
 *     that carry them (RFC 9000 §13.2, §16, §19.3)                                               *
 * ------------------------------------------------------------------------------------------ */

/* rx_track (2k) leaves "which packet numbers have we accepted" in a device table and lists the connections that received
 * something new; tx_seal (2l) starts at "connection c, payload here, packet there".  rx_ack is the step between: for a
 * DEVICE list of connections it writes one ACK frame each from the state entries, packed back to back, and one send request
 * per frame.  d_touched -> rx_ack -> tx_seal needs no host step beyond reading two sums.
 *
 * The frame is RFC 9000 §19.3's, type 0x02 (no ECN counts), a pure function of one entry (next, window) of space `space`:
 *   The accepted set is packet number next - 1 - k for every set bit k of window with k < min(64, next); bits at k >= next are
 *   ignored, not an error.  A run is a maximal stretch of consecutive set bits, taken from bit 0 upwards; run 0 starts at bit 0.
 *   The fields, in order: Largest Acknowledged = next - 1; ACK Delay = ack_delay as given (the caller has applied its
 *   ack_delay_exponent); ACK Range Count r = min(runs behind run 0, max_ranges); First ACK Range = len(run 0) - 1; for
 *   i = 1 .. r: Gap = (clear bits between run i - 1 and run i) - 1, ACK Range Length = len(run i) - 1.  Older runs beyond
 *   max_ranges are dropped (a 64-bit window has at most 31 behind run 0; max_ranges above 31 behaves like 31).
 *   Varints are of minimal length; every range field is below 64 and takes one byte, so the frame has
 *   1 + vl(next - 1) + vl(ack_delay) + 2 + 2 r bytes: 5 .. PTLS_HIP_QUIC_ACK_MAX.
 * The status of list entry j with conn = d_list[j], in this precedence: ACK_NO_CONN for conn >= count; ACK_EMPTY for
 * next == 0; ACK_STATE for next > 2^62 or bit 0 of window clear (the table is the caller's: a corrupt entry must not produce a
 * frame that acknowledges nothing, or a number that cannot exist); else ACK_OK.  Only ACK_OK entries get a frame.
 *
 * After the call exactly n elements of d_status, d_frame_off and d_frame_len are written: d_frame_len[j] = the frame length,
 * 0 unless ACK_OK; d_frame_off[j] = the sum of d_frame_len over the entries before j, for every j.  The frames lie back to back
 * in list order at d_frames + d_frame_off[j]; report->bytes is their sum and exactly that many bytes of d_frames change.  (They
 * are packed, not strided: a typical frame has 5 to 13 bytes against the 81 of the worst case.)  The j'-th ACK_OK entry in list
 * order writes d_reqs[j'] = {data_off = in_off + d_frame_off[j], pkt_off = pkt_base + j' * pkt_stride, conn, len =
 * d_frame_len[j]}; exactly report->n_frames requests are written.  tx_seal takes them as they are, with d_frames lying at
 * in_off inside its d_in: a frame has at least 5 bytes, which meets its sample rule, and whether pkt_stride holds a packet stays
 * with its TX_RANGE.  The state table is not written.  Duplicates in the list are legal, each gets a frame.  The outcome does
 * not depend on the order in which the entries are looked at.  One stream synchronisation, to read the two sums.  n == 0:
 * 0 with both sums 0 and nothing written.
 * The object is only the owner of the scratch and the engine handle, as for rx_track: no loaded entries and no open call are
 * needed.  The scratch is allocated with the first use and grown when a call has more entries: a steady-state call allocates
 * nothing.  Calls on one receive object must be ordered by the caller (same stream).
 * PTLS_HIP_EINVAL, nothing launched and nothing written: a null object, params, report, d_spaces, d_status, d_frame_off,
 * d_frame_len or d_reqs; n != 0 with a null d_list or d_frames; count == 0 or above 2^32 - 1; space > 2; ack_delay >= 2^62;
 * 81 n > 2^32 - 1 (the scan levels are 32-bit); frames_len < 81 n (so that no refusal depends on the data); in_off + 81 n or
 * pkt_base + n * pkt_stride wrapping 2^64.
 * Policy: the call acknowledges every listed connection.  Not answering ACK-only packets with ACK-only packets (RFC 9000
 * §13.2.1) stays the host's duty, through the list it passes.
 * Out of scope: ECN counts (type 0x03); a delay per connection; windows wider than 64; other frames bundled into the same
 * packet; reading received ACK frames into txconn.largest_acked, and knowing whether a packet was ack-eliciting (both need a
 * frame walk over the opened payloads). */
#define PTLS_HIP_QUIC_ACK_MAX 81
#define PTLS_HIP_QUIC_ACK_OK 0u
#define PTLS_HIP_QUIC_ACK_NO_CONN 1u /* the connection lies outside the state table */
#define PTLS_HIP_QUIC_ACK_EMPTY 2u   /* nothing accepted yet in that space */
#define PTLS_HIP_QUIC_ACK_STATE 3u   /* not a state rx_track leaves: next above 2^62, or the largest number not accepted */
typedef struct st_ptls_hip_quic_rx_ack_t { /* 104 bytes */
    const ptls_hip_quic_pnspace_t *d_spaces; /* device: 2k's table, 3 * count entries */
    size_t count;                            /* connections */
    uint32_t space;                          /* 0 Initial, 1 Handshake, 2 0-RTT and 1-RTT */
    uint32_t max_ranges;                     /* ACK ranges to keep behind the first; above 31: 31 */
    uint64_t ack_delay;                      /* the ACK Delay field, below 2^62 */
    void *d_frames;                          /* device: the frames, packed */
    size_t frames_len;                       /* its bytes: at least 81 n */
    uint64_t in_off;                         /* where d_frames lies inside the d_in that tx_seal will get */
    uint64_t pkt_base, pkt_stride;           /* request j' sends its packet to pkt_base + j' * pkt_stride */
    uint32_t *d_status;                      /* device: one PTLS_HIP_QUIC_ACK_* per list entry */
    uint32_t *d_frame_off;                   /* device: one per list entry */
    uint32_t *d_frame_len;                   /* device: one per list entry */
    ptls_hip_quic_txreq_t *d_reqs;           /* device, room for n */
} ptls_hip_quic_rx_ack_t;
typedef struct st_ptls_hip_quic_rx_ack_report_t {
    uint64_t n_frames;
    uint64_t bytes;
} ptls_hip_quic_rx_ack_report_t;
int ptls_hip_quic_rx_ack(ptls_hip_quic_rx_t *rx, const ptls_hip_quic_rx_ack_t *params, const uint32_t *d_list, size_t n,
                         ptls_hip_quic_rx_ack_report_t *report, void *stream);
/* Diagnostic (tools/bench_quic_ack.py): with ptls_hip_quic_rx_timing enabled on the calling thread, the HIP-event time of the
 * last rx_ack's launches (the pointer may be NULL). */
void ptls_hip_quic_rx_ack_timing(float *ack_ms);

/* ------------------------------------------------------------------------------------------ *
 * 3. synthetic workload (bench / tests): the payload of descriptor i is the splitmix64 stream     *
 *    seeded with seed ^ g(i), written at buf + recs[i].in_off for recs[i].len     *
 *    bytes, where g(i) = index[i] if `index` (device array of n uint64) is given, else base + i.     *
 * ------------------------------------------------------------------------------------------ */
int ptls_hip_fill_records(ptls_hip_batch_t *batch, void *buf, uint64_t seed, uint64_t index_base, const uint64_t *index,
                          void *stream);
/* The achievable-HBM reference of the roofline (bench.py): copy `bytes` (a multiple of 16; 16-byte aligned device
 * pointers) from src to dst on the engine's device, one 16-byte load and store per thread, asynchronously on `stream`. */
int ptls_hip_device_copy(ptls_hip_engine_t *engine, void *dst, const void *src, size_t bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
