/*
 * npd.h -- C ABI of libnpd.so, the MI355X-native batch Polar/PAC decoding hot path.
 *
 * The reference (hebbarashwin/neural_polar_decoder) is pure Python/PyTorch with no FFI; its
 * "operator API" for this path is the Python method surface of PolarCode / PAC / RNN_decoder /
 * convNet.  Each entry point below replaces one of those methods (cited per function); the Python
 * mirror in neural_polar_decoder_amd/ binds them with ctypes.
 *
 * Conventions
 *   - All tensor pointers are DEVICE pointers owned by the caller (e.g. torch tensors' data_ptr()),
 *     row-major fp32 unless stated: y/x (B,N), msg/msg_hat (B,K), exactly the reference's layouts.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every call is
 *     stream-ordered and asynchronous; none allocates or synchronises, so calls can be captured
 *     into a hipGraph.
 *   - Handles (npd_code, npd_gru, npd_conv) are immutable after creation: concurrent use from
 *     several host threads on distinct streams is safe.  A handle is bound to the device that was
 *     current when it was created.
 *   - Return value: 0 = success; > 0 = hipError_t passthrough; < 0 = argument error (NPD_E*).
 *     npd_last_error() returns a thread-local description of the last failure.  Nothing aborts.
 *   - Random numbers: Philox4x32-10, counter = (block, stream, codeword index), key = seed, so
 *     results are independent of how codewords are sharded over launches or GPUs.
 */
#ifndef NPD_H_
#define NPD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPD_ABI_VERSION 1

#define NPD_OK 0
#define NPD_EINVAL (-1)   /* bad argument (null pointer, size, unsupported N/K) */
#define NPD_ENOTSUP (-2)  /* configuration not compiled in */
#define NPD_ENOMEM (-3)   /* host allocation failed */

typedef struct npd_code npd_code; /* a Polar or PAC code: N, K, info set, frozen prior, PAC taps */
typedef struct npd_gru npd_gru;   /* a CRISP GRU decoder's weights, repacked for the kernel */
typedef struct npd_conv npd_conv; /* a convNet decoder's weights, repacked for the kernel */

int npd_abi_version(void);
const char* npd_last_error(void);
/* number of visible HIP devices (0 when none); never fails */
int npd_device_count(void);

/* ---------------------------------------------------------------------------------- codes */
/*
 * Create a code.  Replaces PolarCode.__init__ (polar.py:66-117) and PAC.__init__/rate_profiler
 * (pac_code.py:97-174): the caller passes the sorted information set it computed (rate profiles
 * are host logic).  pac_g == 0 -> Polar code; otherwise the PAC convolution polynomial (91 in the
 * reference; its top bit must be set).  infty = the Polar frozen-leaf prior (polar.py:66, default
 * 1000), ignored for PAC (pac_sc_decode applies no prior).  4 <= N <= 256, N a power of two.
 */
int npd_code_create(int N, int K, const int32_t* info_sorted, int pac_g, float infty, npd_code** out);
int npd_code_destroy(npd_code* code);

/* ---------------------------------------------------------------------------------- encode */
/*
 * x = encode(msg).  Polar: PolarCode.encode_plotkin (polar.py:128-148) -- u = ones, u[info] = msg,
 * butterfly left *= right for d = 0..n-1 (bit-exact for any fp32 input, same product order).
 * PAC: PAC.pac_encode (pac_code.py:220-224) -- rate profile, conv pre-transform, rate-1 Plotkin.
 */
int npd_encode(const npd_code* code, const float* msg, float* x, int64_t B, void* stream);

/* ---------------------------------------------------------------------------------- channel */
/*
 * y = x + fl32(sigma) * n, n ~ N(0,1) from Philox stream (seed, snr_index), codeword index
 * cw_offset + b.  Replaces PolarCode.channel / PAC.channel (polar.py:201-207, pac_code.py:226-231).
 * N % 4 == 0.
 */
int npd_awgn(const float* x, float* y, int64_t B, int N, float sigma, uint64_t seed, uint32_t snr_index,
             uint64_t cw_offset, void* stream);

/*
 * Fused Monte-Carlo data generation for codewords cw_offset .. cw_offset+B-1: msg bits from Philox
 * (seed), encode (Polar or PAC), AWGN at (sigma, snr_index).  Any of msg/x may be NULL; y required.
 * Equivalent to msg = 1-2*bits; x = encode(msg); y = channel(x, snr) in the reference eval loops
 * (run_models.py:318-323, rnn_all.py:842-847).
 */
int npd_mc_generate(const npd_code* code, float* msg, float* x, float* y, int64_t B, float sigma, uint64_t seed,
                    uint32_t snr_index, uint64_t cw_offset, void* stream);

/* ---------------------------------------------------------------------------------- SC decode */
/*
 * Successive-cancellation min-sum decoding, one codeword per lane.
 * Polar: PolarCode.sc_decode_new (polar.py:465-484): LLR = llr_scale * y with
 *   llr_scale = fl32(2/sigma^2); f = sign(a)sign(b)min(|a|,|b|) (utils.py:272-275); g = u*a + b;
 *   leaf = L + infty on frozen positions; u = sign(leaf).  Outputs: leaf_llr (B,N) [optional],
 *   msg_hat = u[:, info] (B,K) [optional].  u_hat must be NULL.
 * PAC: PAC.pac_sc_decode (pac_code.py:534-573): same tree, no prior, conv-state leaf rule.
 *   Outputs: leaf_llr (B,N), msg_hat = v_hat[:, info] (B,K), u_hat (B,N); each optional.
 * gt (B,N) optional genie (use_gt polar.py:480 / use_gt_codeword pac_code.py:548-555), else NULL.
 * Decisions and leaf LLRs are bit-exact with the reference (fp32, same operation order).
 */
int npd_sc_decode(const npd_code* code, const float* y, float llr_scale, float* leaf_llr, float* msg_hat,
                  float* u_hat, const float* gt, int64_t B, void* stream);

/*
 * Monte-Carlo SC decode with fused error counting: decodes y (B,N) of codewords
 * cw_offset .. cw_offset+B-1 whose messages are the Philox message stream of `seed` (as written
 * by npd_mc_generate), writes msg_hat (B,K) if non-NULL, and adds {bit errors, block errors} to
 * counters[0..1] (device uint64, not reset).  Error semantics of errors_ber/errors_bler
 * (utils.py:17-51): a decision of 0 counts as an error.
 */
int npd_sc_decode_mc(const npd_code* code, const float* y, float llr_scale, float* msg_hat, uint64_t seed,
                     uint64_t cw_offset, int64_t B, unsigned long long* counters, void* stream);

/*
 * Exact log-sum-exp SC, PolarCode.sc_decode(noisy_code, snr) (polar.py:209-279): check node =
 * log_sum_avoid_zero_NaN (utils.py:295-397), g = u*a + b, frozen leaves decided +1 (no prior),
 * information leaves sign(L) (hard_decision != 0, args.hard_decision) or tanh(L/2) (hard_decision == 0,
 * the reference's default).  Outputs (each optional): msg_hat = sign(decoded_bits)[:, info] (B,K) and
 * u_bits = decoded_bits (B,N).  Polar codes, N <= 256.  exp/log/tanh are the device libm, so values
 * agree with torch's CPU path to a few ulp (decisions except on near-zero LLRs).
 */
int npd_sc_decode_lse(const npd_code* code, const float* y, float llr_scale, int hard_decision, float* msg_hat,
                      float* u_bits, int64_t B, void* stream);

/*
 * Soft-output SC, PolarCode.sc_decode_soft(noisy_code, snr, priors) (polar.py:281-358): LSE check
 * nodes, leaf L^ = clamp(L + prior, -1000, 1000), right-child input LSE(L^_left, L_a) + L_b, nodes
 * return [LSE(L^_u, L^_v), L^_v]; frozen positions get no special treatment (priors carry them).
 * priors: HOST array of N floats or NULL (zeros).  Outputs as npd_sc_decode_lse.  4 <= N <= 256, y
 * 16-byte aligned.
 */
int npd_sc_decode_soft(const npd_code* code, const float* y, float llr_scale, int hard_decision, const float* priors,
                       float* msg_hat, float* u_bits, int64_t B, void* stream);

/*
 * PolarCode.sc_decode_soft_new(corrupted_codewords, snr, priors) (polar.py:485-607: updateLLR_soft,
 * partial_decode_soft, updatePartialSums_soft): SC whose partial sums are LLRs ("soft partial sums",
 * [a, b] -> [LSE(a, b), b] per stage) -- the decode_soft recursion above -- with the leaf stored as
 * clamp(L + prior, +-1000) + prior.  Outputs msg_hat (B,K) = sign(stored leaf)[:, info] (the reference's
 * return value) and optionally u_hat (B,N) = sign of every stored leaf.  priors (N floats, host) or NULL
 * (zeros: frozen positions are decided like information positions, as in the reference).  Polar codes,
 * 4 <= N <= 256, y 16-byte aligned.
 */
int npd_sc_decode_soft_new(const npd_code* code, const float* y, float llr_scale, const float* priors, float* msg_hat,
                           float* u_hat, int64_t B, void* stream);

/* ---------------------------------------------------------------------------------- SC-List decode */
/*
 * Successive-cancellation list decoding, PolarCode.scl_decode(y, snr, L, use_CRC=False)
 * (polar.py:793-876) with pruneLists (polar.py:777-791): min-sum SC per path (no frozen prior in the
 * LLRs), path metric += |leaf| on a frozen leaf with sign(leaf) != 1 and on the flipped branch of an
 * information leaf; survivors = torch.topk's choice (ties resolved exactly as std::nth_element, see
 * npd_list_prune_select) in list order; final path = the first minimum of ||encode(u) - y||^2.
 * Polar and PAC codes, 8 <= N <= 256, 1 <= list_size <= 32 (any value, not only powers of two; the live list is
 * min(2^bits decided, list_size) paths, the final one min(2^K, list_size)), y 16-byte aligned.  Outputs: msg_hat (B,K) and
 * u_hat (B,N) of the chosen path, each optional.  scl_decode's leaf-LLR output equals
 * npd_sc_decode(..., gt = u_hat) (a genie pass reproduces the chosen path's LLRs bit for bit).
 * Decisions are bit-exact with the reference except when two list candidates' fp32 distances differ
 * only by summation order (torch's vectorised sum vs a sequential one here).
 *
 * PAC handles (pac_g > 1; the reference has no PAC list decoder, so this defines one): the same list decoder with
 * its leaf step replaced by pac_sc_decode's (pac_code.py:534-573); no priors.  Every path also carries its
 * convolution state, the last len(g_array) - 1 values of v_hat, initially all +1; u0 = conv1bTrans(+1, state) is the
 * product of the tapped state entries (conv1bTrans(-1, state) = -u0).
 *   frozen position:      v = +1, u = u0, the state advances with +1; metric = fl32(m + |l|) if sign(l) != u0
 *                         (sign(0) = 0 counts as unequal, the penalty is then 0), else m; no fork.
 *   information position: every path forks, in list order, into [keep_0 .. keep_{s-1}, flip_0 .. flip_{s-1}]; keep has
 *                         u = sign(l), metric m; flip has u = -sign(l), metric fl32(m + |l|); v = u * u0 advances the
 *                         state; l == 0 gives u = v = 0 in both children and the state does not advance.  More than
 *                         list_size children are pruned as above.
 *   final path:           the first minimum over the live list of ||polar_encode(u) - y||^2 (fp32, summed sequentially).
 * For PAC msg_hat is v_hat[:, B] and u_hat is the convolved word u; the fused counts of npd_scl_decode_mc compare
 * v_hat[:, B] with the Philox message (a 0 counts as an error).  list_size = 1 is pac_sc_decode bit for bit; pac_g = 2
 * (no tap, u = v) gives Polar SC-List's decisions.
 */
int npd_scl_decode(const npd_code* code, const float* y, float llr_scale, int list_size, float* msg_hat,
                   float* u_hat, int64_t B, void* stream);
/* Monte-Carlo SC-List decode with fused error counting (semantics of npd_sc_decode_mc). */
int npd_scl_decode_mc(const npd_code* code, const float* y, float llr_scale, int list_size, float* msg_hat,
                      uint64_t seed, uint64_t cw_offset, int64_t B, unsigned long long* counters, void* stream);
/*
 * Host utility (no GPU): the survivor set of pruneLists for n <= 16 candidates whose negated metrics
 * are neg_metrics[0..n) in list order, keeping `keep` -- bit c of *mask_out set iff candidate c
 * survives.  The same code runs inside the SCL kernel when metrics tie across the boundary.
 */
int npd_list_prune_select(const float* neg_metrics, int n, int keep, uint32_t* mask_out);
/* The same for 1 <= keep <= n <= 64 candidates (list sizes 9 .. 32 prune up to 64), as a 64-bit mask. */
int npd_list_prune_select64(const float* neg_metrics, int n, int keep, uint64_t* mask_out);

/* ---------------------------------------------------------------------------------- CRC-aided SC-List decode */
/*
 * PolarCode.scl_decode(y, snr, L, use_CRC=True) (polar.py:849-866) with get_CRC / CRC_check / encode_with_crc
 * (polar.py:738-775).  The reference's helpers do not run as written (they read a module global that exists only when
 * polar.py is the script) and, once they do, attach the CRC with the opposite bit convention to the one CRC_check
 * reads, so a correctly received word never passes.  This project therefore defines the decoder, taking from the
 * reference what is well defined: the polynomial division (polar.py:738-748), its three polynomials and the selection
 * rule (polar.py:860-866).  Polar and PAC codes.
 *
 * Polynomial.  crc_poly: bit i is the coefficient of x^i; the degree c is the index of the top set bit.  Rules:
 *   1 <= c <= 24, bit 0 set, c < K; anything else returns NPD_EINVAL.  The reference's polynomials are 0xB (c = 3),
 *   0x1D5 (c = 8) and 0x11021 (c = 16).
 * Bits.  Symbol -1 is bit 1 and +1 is bit 0, the convention of the Philox messages (msg = 1 - 2 bit).  A decision of 0
 *   is neither.
 * CRC.  The K information slots, in the order of the sorted information set (the column order of msg), carry
 *   m_0 .. m_{K-c-1} and then r_0 .. r_{c-1}, where r(x) = (sum_k m_k x^(K-c-1-k)) x^c mod g(x) and r_i is the
 *   coefficient of x^(c-1-i): the plain division, MSB first, zero initial register, no reflection, no final XOR.  For
 *   PAC codes the CRC covers the message before the convolution (pac_encode([msg, crc])).
 * A path passes if its K information decisions (Polar: u_hat at the information set; PAC: v_hat there) contain no 0
 *   and, read as a polynomial of degree K - 1, leave remainder 0.
 * Selection (polar.py:860-866).  Over the live list of min(2^K, list_size) paths in list order: the passing path of
 *   smallest path metric, the first in list order on a tie; if no path passes, the path of smallest metric, the first
 *   in list order on a tie; crc_ok = 1 or 0 accordingly.  Nothing else about the list changes: forking, metrics,
 *   pruning and tie rules are those of npd_scl_decode; the distance step is not run.  (The tie rules are those of the
 *   (value, index) reduction that npd_scl_decode's final step uses; no word set tried produced two passing paths tied
 *   at the minimum, so no test exercises that one.)
 *
 * npd_crc_attach: out (B,K) = [msg (B,K-c) unchanged | the CRC columns as +-1, computed from bit = msg < 0].
 * npd_mc_generate_crc: npd_mc_generate whose message bits 0 .. K-c-1 are the Philox message stream and whose bits
 *   K-c .. K-1 are their CRC; the first K-c message columns and the noise are exactly those npd_mc_generate gives.
 *   msg (B,K) and x optional, y required.
 * npd_scl_decode_crc: limits of npd_scl_decode (Polar and PAC handles, 8 <= N <= 256, 1 <= list_size <= 32, y 16-byte
 *   aligned).  Outputs of the chosen path, each optional but at least one: msg_hat (B,K) (the CRC columns included),
 *   u_hat (B,N), crc_ok (B) int32.  The chosen path's leaf LLRs are npd_sc_decode(..., gt = u_hat), as for
 *   npd_scl_decode.
 * npd_scl_decode_crc_mc: decode and count in one launch; counters[0..2] (device uint64, not reset) += {bit errors over
 *   the K-c message bits against the Philox message (a 0 counts as an error), block errors over the same K-c bits,
 *   words with crc_ok == 0}.
 * All four check every pointer and the polynomial before any HIP call, are stream-ordered, allocate nothing, and
 * return NPD_OK for B = 0.
 */
int npd_crc_attach(const float* msg, float* out, int64_t B, int K, uint32_t crc_poly, void* stream);
int npd_mc_generate_crc(const npd_code* code, uint32_t crc_poly, float* msg, float* x, float* y, int64_t B, float sigma,
                        uint64_t seed, uint32_t snr_index, uint64_t cw_offset, void* stream);
int npd_scl_decode_crc(const npd_code* code, const float* y, float llr_scale, int list_size, uint32_t crc_poly,
                       float* msg_hat, float* u_hat, int32_t* crc_ok, int64_t B, void* stream);
int npd_scl_decode_crc_mc(const npd_code* code, const float* y, float llr_scale, int list_size, uint32_t crc_poly,
                          float* msg_hat, uint64_t seed, uint64_t cw_offset, int64_t B, unsigned long long* counters,
                          void* stream);

/*
 * A whole SNR sweep of npd_sc_decode_mc in one launch: y is (n_snr, B, N) -- the received words of
 * the same codewords cw_offset .. cw_offset+B-1 at n_snr SNR points (the reference's per-SNR loop,
 * run_models.py:318-371), llr_scale a HOST array of n_snr scales, msg_hat (n_snr, B, K) or NULL,
 * counters (n_snr, 2).  1 <= n_snr <= 16.  Same results as n_snr separate npd_sc_decode_mc calls.
 */
int npd_sc_decode_mc_sweep(const npd_code* code, int n_snr, const float* y, const float* llr_scale, float* msg_hat,
                           uint64_t seed, uint64_t cw_offset, int64_t B, unsigned long long* counters, void* stream);

/*
 * The Monte-Carlo step in one launch, y never stored: for each of the n_snr segments s and codeword
 * cw_offset .. cw_offset+B-1, the message (Philox message stream of `seed`), its codeword and the
 * received word (noise stream snr_index0 + s, sigma[s]) are generated in registers exactly as
 * npd_mc_generate writes them, SC-decoded with llr_scale[s] and counted into counters (n_snr, 2)
 * (and msg_hat (n_snr, B, K) if non-NULL).  Equal, count for count, to npd_mc_generate (snr_index =
 * snr_index0 + s) followed by npd_sc_decode_mc_sweep.  sigma and llr_scale are HOST arrays.  Polar
 * codes with 8 <= N <= 64 (NPD_ENOTSUP otherwise).  Replaces the generate/decode/count body of the
 * reference's eval loops (run_models.py:318-337, rnn_all.py:842-856) for the SC decoder.
 */
int npd_sc_mc_sweep_fused(const npd_code* code, int n_snr, const float* sigma, const float* llr_scale,
                          uint32_t snr_index0, uint64_t seed, uint64_t cw_offset, int64_t B, float* msg_hat,
                          unsigned long long* counters, void* stream);

/* ---------------------------------------------------------------------------------- ML / bitwise MAP */
/*
 * Decoding against the whole codebook, the "ML" and "bitML" curves of the reference's eval loops
 * (run_models.py:347-361 and :1374-1377; rnn_all.py:892-948 under --run_ML).  Stateless on an npd_code: the codebook is
 * never stored -- the kernels XOR K generator rows (computed on the host inside the call) into the sign bits of
 * fp16 MFMA fragments.  Polar and PAC codes, N in {8, 16, 32, 64}; ML 1 <= K <= 22, MAP 1 <= K <= 16; anything else
 * returns NPD_ENOTSUP (npd_ml_supported tells beforehand: 1 / 0, < 0 on NULL; map != 0 asks for npd_map_decode).
 *
 * Codeword index i follows dec2bitarray (utils.py:170-192), MSB first: message column k of index i is
 * 1 - 2 * ((i >> (K-1-k)) & 1), so index 0 is the all-(+1) message and all_message_bits[i] (run_models.py:1349-1356)
 * is row i of the codebook's messages.
 *
 * npd_ml_decode: idx[b] = argmax_i sum_j y[b][j] c_i[j], which is the reference's
 *   diff = (b_noisy - b_codebook).pow(2).sum(2); idx = diff.argmin(1); decoded = all_message_bits[idx]
 *   (run_models.py:348-351).  Outputs, each optional but at least one: msg_hat (B,K) = all_message_bits[idx],
 *   idx (B) int32, metric (B) = the chosen codeword's correlation (re-summed in fp64, rounded once).
 *   Among codewords whose computed correlations are equal and maximal the smallest index wins (torch.argmin's first
 *   occurrence).  The correlations are sums of exact products (y split into three fp16 planes) accumulated in fp32:
 *   the chosen codeword's exact correlation is within 2 N 2^-24 sum_j |y_j| of the best one.
 * npd_map_decode: PolarCode.bitwise_MAP (polar.py:879-899) -- with a = llr_scale * y (llr_scale = 2/sigma^2 >= 0),
 *   llr[b][k] = logsumexp_{i: bit_k(i) = 0} a.c_i - logsumexp_{i: bit_k(i) = 1} a.c_i and
 *   msg_hat[b][k] = +1 if llr >= 0 else -1 (torch.max's first index on a tie).  Outputs msg_hat (B,K) and llr (B,K),
 *   each optional but at least one.  Defined for PAC codes in the same way (the reference has no PAC bitwise_MAP).
 */
int npd_ml_supported(const npd_code* code, int map);
int npd_ml_decode(const npd_code* code, const float* y, float* msg_hat, int32_t* idx, float* metric, int64_t B,
                  void* stream);
int npd_map_decode(const npd_code* code, const float* y, float llr_scale, float* msg_hat, float* llr, int64_t B,
                   void* stream);

/* ---------------------------------------------------------------------------------- counters */
/*
 * counters[0] += #(round(ref) != round(hat)), counters[1] += #rows with any such element, over
 * (B,K) fp32 arrays.  Replaces errors_ber / errors_bler's counting (utils.py:17-51) with device
 * uint64 counters (no host sync per batch).
 */
int npd_count_errors(const float* ref, const float* hat, int64_t B, int K, unsigned long long* counters,
                     void* stream);

/*
 * As npd_count_errors, comparing ref (B,K) with columns cols[0..K) (HOST array, each < W) of hat (B,W):
 * the reference's `errors_ber(msg, decoded[:, info])` (rnn_all.py:874-879, run_models.py:333-337)
 * without materialising the gathered (B,K) copy.  K <= 256.
 */
int npd_count_errors_cols(const float* ref, const float* hat, int64_t B, int K, int W, const int32_t* cols,
                          unsigned long long* counters, void* stream);

/*
 * errors_ber(ref, hat, mask) with an integer mask (utils.py:17-25; the loops pass torch.ones(...).long(),
 * run_models.py:325-341): counters[0] += sum(mask * (round(ref) != round(hat))), counters[1] += sum(mask),
 * over (B,K) arrays (mask int64).  errors_ber = counters[0] / counters[1], decided on the device (no host
 * read of the mask).
 */
int npd_count_errors_masked(const float* ref, const float* hat, const int64_t* mask, int64_t B, int K,
                            unsigned long long* counters, void* stream);

/* ---------------------------------------------------------------------------------- CRISP GRU */
/*
 * Create a GRU decoder from an RNN_Model state dict (rnn_all.py:294-398): nn.GRU(input_size, F,
 * layers, batch_first) + Linear(F, 1), decoding_type y_input without the y-MLP.
 * weights: host fp32, packed per layer l = 0..layers-1 as
 *   weight_ih_l (3F, Din_l) | weight_hh_l (3F, F) | bias_ih_l (3F) | bias_hh_l (3F),
 * then linear.weight (F) | linear.bias (1); Din_0 = N + 2 (onehot) or N + 1, Din_l = F for l > 0.
 * precision: 0 = fp32 (default, exact fp32 FMA chains), 1 = bf16x3 split, 2 = bf16, 3 = fp16x3 split (hi + lo fp16
 * parts, three products per multiply, fp32 accumulation: held to the fp32 path's tolerance; F <= 64).
 * N: a multiple of 8 in [8, 256] (split precisions: of 16).  F > 64 keeps both layers' states and the tile's y in LDS,
 * (layers F + N + min(F / 32, 8)) * 128 bytes <= 160 KiB: only F = 512 with 2 layers is bounded by it, to N <= 248.
 */
int npd_gru_create(int N, int F, int layers, int onehot, const float* weights, int64_t n_weights, int precision,
                   npd_gru** out);
int npd_gru_destroy(npd_gru* gru);
/*
 * npd_gru_create for either cell of rnn_all.py:69 (--rnn_type GRU | LSTM): cell 0 = GRU (npd_gru_create), cell 1 =
 * LSTM (nn.LSTM, gates i, f, g, o; the same weight order with 4F gate rows: weight_ih_l (4F, Din_l) | weight_hh_l (4F, F)
 * | bias_ih_l (4F) | bias_hh_l (4F) per layer, then linear.weight | linear.bias).  LSTM: fp32 (precision 0), hidden
 * 32, 64, 128, 256 or 512, 1 or 2 layers (F = 512 with 2 layers: N <= 248, the GRU's LDS bound), y_input decoding
 * (npd_gru_decode) or y_h0 decoding (npd_gru_decode_ex with y = NULL: h and c both start from h0, as get_h0 returns
 * (x, x) for LSTM, rnn_all.py:370-375); destroy with npd_gru_destroy.
 */
int npd_rnn_create(int cell, int N, int F, int layers, int onehot, const float* weights, int64_t n_weights, int precision,
                   npd_gru** out);
/*
 * npd_rnn_create with the reference's other output heads (rnn_all.py:317-343; forward rnn_all.py:387-398: decoded =
 * linear(layernorm(out))).  GRU cells, fp32 (precision 0), F 32 or 64 (gru_decode_kernel), unidirectional.
 *  - --use_layernorm: ln_weight / ln_bias (F, host) are nn.LayerNorm(F)'s gamma / beta, ln_eps its eps.  The affine part
 *    folds into the output Linear (w gamma, b + w . beta); the kernel normalises each step's top-layer state (two-pass
 *    mean and biased variance over the F units).  ln_weight = NULL: no LayerNorm.
 *  - --out_linear_depth > 1 (head_depth): linear = Linear(F, H), SELU, [Linear(H, H), SELU] x (depth - 2), Linear(H, 1)
 *    with H = head_hidden (the net's y_hidden_size, 1 .. 128); head_weights (host) = the Linear layers' weight and
 *    bias in order (W_0 (H, F), b_0 (H), ..., W_last (1, H), b_last (1)), n_head values; the last F + 1 values of
 *    `weights` (the depth-1 linear) are then ignored.  Each head layer is an fp32 MFMA GEMM per step inside the decode
 *    loop.  head_depth = 1: the plain Linear(F, 1) of `weights`.  Not combined with the LayerNorm.
 * ln_weight = NULL and head_depth = 1 is npd_rnn_create.
 */
int npd_rnn_create_ex(int cell, int N, int F, int layers, int onehot, const float* weights, int64_t n_weights,
                      int precision, const float* ln_weight, const float* ln_bias, float ln_eps, int head_depth,
                      int head_hidden, const float* head_weights, int64_t n_head, npd_gru** out);
/*
 * RNN_decoder.decode(net, False, y, gt) test branch (rnn_all.py:532-547): decoded (B,N) fp32, with
 * decoded[:, i] = sign(out_i) for i in the info set (is_info: N bytes, host) and 1 (or gt) else.
 * reverse: RNN_decoder reverse_order (rnn_all.py:414-416).  logits (B,N) optional: raw output at
 * every step.
 */
int npd_gru_decode(const npd_gru* gru, const float* y, const uint8_t* is_info, int reverse, const float* gt,
                   float* decoded, float* logits, int64_t B, void* stream);
/*
 * The same decode with an initial state and an optional y input -- decoding_type 'y_h0' (rnn_all.py:523-531):
 * hidden = net.get_h0(y), then every step's RNN input is onehot(previous decision) alone.  The handle is created
 * from weights whose weight_ih_l0 carries N zero columns before the one-hot / sign columns (the y_input layout with
 * the y part zero); y = NULL skips that projection.  h0: (B, F * layers) fp32 on the device, element f * layers + l =
 * layer l, hidden unit f -- get_h0's x before its reshape(-1, F, layers).permute(2, 0, 1) (rnn_all.py:362-375).
 * Precision 0, or the 16-codeword split kernel (F = 64, 2 layers, N % 32 == 0); y = NULL and h0 = NULL is an error.
 * LSTM handles take exactly one of y (y_input) and h0 (y_h0, both states start from it), fp32.
 */
int npd_gru_decode_ex(const npd_gru* gru, const float* y, const float* h0, const uint8_t* is_info, int reverse,
                      const float* gt, float* decoded, float* logits, int64_t B, void* stream);
/*
 * The eval loop's GRU half over an SNR sweep (rnn_all.py:853-880: at each SNR point decoded = RNN_decoder.decode(y_s),
 * then errors_ber / errors_bler(msg, decoded[:, info]), rnn_all.py:874-879, utils.py:17-51): y is (n_seg, B, N), one
 * segment of received words per SNR point; msg (B, K) the message bits of the B codewords (the same messages in every
 * segment: the Monte-Carlo driver's message stream is keyed by codeword, not SNR); cols (K, HOST) the decoded columns
 * compared with msg's columns, K <= N distinct positions in any order (a repeat is NPD_EINVAL; K = N = 256 compares
 * every position, message column 255 included).  counters (n_seg, 2) += [bit errors, block errors] of each segment --
 * equal, count for count, to npd_gru_decode_ex + npd_count_errors_cols per segment.  decoded (n_seg, B, N) is optional for the
 * 16-codeword split kernel (F = 64, 2 layers, N % 32 == 0, precision != 0), which decodes and counts every segment in
 * ONE launch (errors counted in the decision epilogue, one atomic pair per wave and segment); other handles run one
 * decode + one count per segment and need decoded.  y_input decoding, no gt, no logits.
 */
int npd_gru_decode_count_sweep(const npd_gru* gru, int n_seg, const float* y, const uint8_t* is_info, int reverse,
                               const float* msg, int K, const int32_t* cols, float* decoded, int64_t B,
                               unsigned long long* counters, void* stream);
/*
 * CRISP GRU list decoding, RNN_decoder.list_decode(net, y, code, L) (rnn_all.py:563-664, decoding_type y_input) with
 * its pruneLists (rnn_all.py:563-578): list_size partial decodings per word; every live path runs one GRU step per
 * position on [fy, onehot(its previous bit)] (+1 at step 0 and after a frozen position); a frozen position only
 * advances the state (bit +1, no metric penalty, unlike SCL); an information position forks each path into
 * sign(out) (metric unchanged) and -sign(out) (metric + |out|, fp32 in step order), both on the same new state, and
 * when more than list_size children exist the survivors are torch.topk's choice (ties resolved exactly as
 * std::nth_element, see npd_list_prune_select; a NaN metric ranks as topk ranks it) in ascending child order.  The
 * final path is the first minimum over the list of ||encode(msg) - y||^2 with the code's own encoder (Polar: Plotkin
 * transform; PAC: rate-1 convolution, then the transform).
 * y (B,N): the received words, used for the final selection; fy (B,N): the GRU's input, or NULL to use y (nets with a
 * y-MLP pass its output, RNN_Model.get_Fy); both 16-byte aligned.  The information set and the encoder come from
 * `code` (Polar or PAC), whose N must equal the handle's.  1 <= list_size <= 8 (any value, not only powers of two);
 * there are min(list_size, 2^K) survivors.
 * Outputs, each optional but at least one of msg_hat and cand_msg: msg_hat (B,K) the chosen survivor's message (+-1),
 * sel (B) int32 its index in list order, cand_msg (B, list_size, K) and cand_metric (B, list_size) the final list in
 * the reference's order; unused slots (2^K < list_size) carry metric +inf and message 0.
 * One launch, no allocation, no host synchronisation; B = 0 returns NPD_OK.  Runs on the fp32 kernels: GRU handles
 * with precision 0, 1 or 2 layers and the plain Linear(F, 1) head, at F 32 or 64 (weights in LDS) and at F 256 or 512
 * (weights streamed, as npd_gru_decode at those widths, with its N limit) -- LSTM, split-precision, F = 128,
 * LayerNorm-head and out_linear_depth > 1 handles return NPD_ENOTSUP (npd_gru_list_supported tells beforehand:
 * 1 / 0, < 0 on NULL).  list_size = 1 is npd_gru_decode's greedy decision, bit for bit, at every width.
 * Decisions follow the reference's arithmetic in fp32 (gate nonlinearities to ~1 ulp, as npd_gru_decode), so a
 * survivor set can differ where two metrics are closer than the logits' tolerance, and two candidates whose fp32
 * distances differ only by summation order (torch's vectorised sum vs the kernel's) may swap in the final selection.
 */
int npd_gru_list_supported(const npd_gru* gru, const npd_code* code, int list_size);
int npd_gru_list_decode(const npd_gru* gru, const npd_code* code, const float* y, const float* fy, int list_size,
                        float* msg_hat, int32_t* sel, float* cand_msg, float* cand_metric, int64_t B, void* stream);
/*
 * CRC-aided CRISP GRU list decoding.  The reference has no such decoder (its CRC helpers do not run and its
 * list_decode takes no CRC), so, as for CRC-aided SC-List decode above, this header defines it.
 * Polynomial, bit convention and CRC layout are exactly those of "CRC-aided SC-List decode": crc_poly bit i is the
 *   coefficient of x^i, 1 <= c <= 24, bit 0 set, c < K (anything else NPD_EINVAL); symbol -1 is bit 1; the K information
 *   slots in sorted-information-set order carry K-c message bits and then the c CRC bits; for PAC codes the CRC covers
 *   the message before the convolution, i.e. the path's v bits.
 * The list is npd_gru_list_decode's, bit for bit: forking, metrics, pruneLists, tie rules and list order.
 * A path passes if its K information bits, read as a polynomial of degree K-1, leave remainder 0 (list paths hold +-1
 *   only, so there is no 0 decision).  Unused slots (2^K < list_size) do not pass.
 * Selection.  The first minimum, in list order, of ||encode(msg) - y||^2 -- the same fp32 distance the plain epilogue
 *   computes -- over the passing live paths; if no live path passes, the first minimum over all live paths, which is
 *   exactly npd_gru_list_decode's choice; crc_ok = 1 or 0 accordingly.  The rule is distance, not metric: the GRU
 *   list's metrics are sums of |out| penalties, not likelihoods, and the plain decoder already chooses by distance;
 *   the CRC only restricts the candidate set.  A caller who wants another rule takes the candidates.
 * npd_gru_list_decode_crc outputs, each optional but at least one of msg_hat and cand_msg: msg_hat (B,K) (the CRC
 *   columns included, as npd_scl_decode_crc), sel (B) and crc_ok (B) int32, cand_msg (B, list_size, K) and cand_metric
 *   (B, list_size) as npd_gru_list_decode, cand_crc (B, list_size) int32: each candidate's remainder register (0: it
 *   passes), -1 for unused slots.  crc_poly = 0 is NPD_EINVAL.
 * npd_gru_list_decode_crc_mc decodes, chooses and counts in one launch: counters[0..2] (device uint64, not reset) +=
 *   {bit errors over the K-c message bits against the Philox message of (seed, cw_offset + word), as
 *   npd_scl_decode_crc_mc regenerates it; block errors over the same bits; words with crc_ok == 0}.  msg_hat (B,K) is
 *   optional.  Here only, crc_poly = 0 is allowed: plain selection (npd_gru_list_decode's), counts over all K bits,
 *   counters[2] untouched.
 * Limits and error behaviour are npd_gru_list_decode's: the same handles (NPD_ENOTSUP for those the list kernels
 * refuse), 1 <= list_size <= 8, y / fy 16-byte aligned, NULL and polynomial checks before any HIP call, stream-ordered,
 * no allocation, B = 0 returns NPD_OK.
 */
int npd_gru_list_decode_crc(const npd_gru* gru, const npd_code* code, const float* y, const float* fy, int list_size,
                            uint32_t crc_poly, float* msg_hat, int32_t* sel, int32_t* crc_ok, float* cand_msg,
                            float* cand_metric, int32_t* cand_crc, int64_t B, void* stream);
int npd_gru_list_decode_crc_mc(const npd_gru* gru, const npd_code* code, const float* y, const float* fy, int list_size,
                               uint32_t crc_poly, float* msg_hat, uint64_t seed, uint64_t cw_offset, int64_t B,
                               unsigned long long* counters, void* stream);
/*
 * One layer of RNN_Model.get_h0 / get_Fy (rnn_all.py:362-385): out (B, Nout) = act(x (B, K) W^T + bias), W (Nout, K)
 * row-major, all device fp32, k summed in order.  act: 0 linear, 1 relu, 2 selu, 3 elu, 4 tanh, 5 sigmoid
 * (RNN_Model.act, rnn_all.py:346-360).  get_h0 follows layer ii with act iff ii != y_depth (rnn_all.py:364-368): every
 * layer, the last included, when y_depth >= 2; all but the last when y_depth = 1 (two layers) -- the caller passes
 * act = 0 for that one layer.
 */
int npd_ymlp_layer(const float* x, const float* W, const float* bias, float* out, int64_t B, int K, int Nout, int act,
                   void* stream);

/* ---------------------------------------------------------------------------------- CRISP GRU training */
typedef struct npd_gru_train npd_gru_train; /* the plan of one shape: the device buffers of the kernels' weight images */
/*
 * RNN_decoder.decode(net, True, y, gt, teacher_forcing_ratio) (rnn_all.py:422-512), differentiable: decoding_type
 * y_input without the y-MLP, GRU cells, unidirectional, the plain Linear(F, 1) head, no LayerNorm, no dropout, fp32.
 * N a multiple of 8 in [8, 256], F 32 or 64, 1 or 2 layers (anything else NPD_EINVAL).  The plan holds no weights: every
 * call takes them as one flat DEVICE vector in npd_gru_create's order (per layer weight_ih | weight_hh | bias_ih |
 * bias_hh, then linear.weight | linear.bias) and packs its images from it on the device, so a call after an optimiser
 * step sees the new weights with no host copy and no synchronisation.  One plan serves one stream at a time.
 * npd_gru_train_destroy(NULL) is an argument error (NPD_EINVAL), not a no-op.
 */
int npd_gru_train_create(int N, int F, int layers, int onehot, npd_gru_train** out);
int npd_gru_train_destroy(npd_gru_train* plan);
/*
 * Sizes (in floats) of the two caller-owned device buffers of a batch of B words: `saved` (forward writes, backward
 * reads: per step and layer h', r, z, n and W_hn h + b_hn, and the fed inputs: N B (5 layers F + 3) floats) and `scratch`
 * (backward's own: the gate gradients, N B (4 F layers + 1) floats, and the contraction's partial sums).  Both must be
 * 16-byte aligned; their layout is the library's.
 */
int npd_gru_train_workspace(const npd_gru_train* plan, int64_t B, int64_t* saved_floats, int64_t* scratch_floats);
/*
 * Forward, everything in the step frame ii = 0 .. N-1 (under reverse_order the caller flips gt before and out after).
 * Step 0 is fed +1; step ii + 1 is fed bits[:, ii] = gt[:, ii] (student = 0, values in {-1, 0, +1}) or
 * sign(out[:, ii]) (student = 1); with onehot, -1 and 0 feed column 0 and +1 column 1 (get_onehot).  out[:, ii] is step
 * ii's logit where writes_logit[ii] (HOST, N bytes) is set and the constant 1.0 elsewhere (student forcing writes
 * the information steps only, rnn_all.py:493; teacher forcing every step).  y, gt, out, bits: device (B, N) fp32, y
 * 16-byte aligned; gt may be NULL when student = 1.  Two launches (image packing, the fused N-step forward); B = 0
 * returns NPD_OK with no launch.
 */
int npd_gru_train_forward(npd_gru_train* plan, const float* weights_dev, const float* y, const float* gt_or_null,
                          const uint8_t* writes_logit, int student, float* out, float* bits, float* saved, int64_t B,
                          void* stream);
/*
 * Backward of the forward that filled `saved` (same weights_dev, y, B): grad_out (B, N) device, step frame, and 0 where
 * the forward wrote no logit.  grad_weights_dev (flat, the weights' order and length) is OVERWRITTEN with the gradient
 * of sum(grad_out * out).  Four launches: image packing, the fused backward recurrence, the weight-gradient
 * contraction into per-workgroup partial sums and their reduction in a fixed order (no floating-point atomics: equal
 * calls return equal bits).  B = 0 zeroes the gradient.
 */
int npd_gru_train_backward(npd_gru_train* plan, const float* weights_dev, const float* y, const float* grad_out,
                           const float* saved, float* scratch, float* grad_weights_dev, int64_t B, void* stream);

/* ---------------------------------------------------------------------------------- conv model */
/*
 * convNet (models.py:691-772) forward/decode.  weights: host fp32 in state_dict order
 * (layers1.0.weight, layers1.0.bias, ..., layersFin.4.bias, layer_norm.weight, layer_norm.bias).
 * embed = config.embed_dim (even), N = config.N = config.max_len.
 * precision: 0 = fp32 (exact fp32 FMA chains); 3 = fp16x3 (conv layers with cin > 1 and the Linear layers: hi + lo
 * fp16 operands on the fp16 MFMA, three products per multiply, fp32 accumulation, weights scaled by 2^SW per layer
 * and activations by 2^4 before the split; layer 0, epilogues and LayerNorm fp32).
 */
int npd_conv_create(int N, int embed, const float* weights, int64_t n_weights, int precision, npd_conv** out);
int npd_conv_destroy(npd_conv* conv);
/* logits (B,N) and/or decoded = sign(logits) (B,N); workspace sized by npd_conv_workspace_bytes */
int64_t npd_conv_workspace_bytes(const npd_conv* conv, int64_t B);
int npd_conv_forward(const npd_conv* conv, const float* y, float* logits, float* decoded, void* workspace,
                     int64_t B, void* stream);
/* As npd_conv_forward, and (if input4 != NULL) the intermediate activation convNet.forward also returns,
 * input4 = layers3(input3) + input3 (models.py:750, :767), channels-first (B, embed/2, N) fp32. */
int npd_conv_forward_ex(const npd_conv* conv, const float* y, float* logits, float* decoded, float* input4,
                        void* workspace, int64_t B, void* stream);
/* As npd_conv_forward, and (if tap_out != NULL) one intermediate activation, fp32, in the reference's layout:
 * tap 0 .. 9: the output of conv layer tap (layers1.0, layers1.2, layers2.0, ..., layers5.2) after GELU and, where the
 * layer closes a residual block (3, 5, 7), after the residual, channels-first (B, cout, N); tap 10, 11, 12: the
 * outputs of layersFin.0 / .2 (after GELU) and layersFin.4 (before LayerNorm), (B, 4N), (B, N), (B, N).
 * npd_conv_forward_ex is tap = 5. */
int npd_conv_forward_tap(const npd_conv* conv, const float* y, float* logits, float* decoded, int tap, float* tap_out,
                         void* workspace, int64_t B, void* stream);

/* ---------------------------------------------------------------------------------- conv model training */
typedef struct npd_conv_train npd_conv_train; /* the plan of one (N, embed): the device buffers of the weight images */
/*
 * convNet.forward in training mode (models.py:742-767), differentiable, fp32 (exact fp32 FMA chains on the fp32 MFMA;
 * the fp16x3 split has no training kernels).  N a multiple of 64 in [64, 1024], embed a multiple of 16 in [16, 512]
 * (anything else NPD_EINVAL); embed > 448 is refused with NPD_ENOTSUP (layer 8's dX slab would pass 160 KB of LDS).
 * The plan holds no weights: every call takes all parameters as one flat DEVICE fp32 vector in npd_conv_create's
 * order (per conv layer w then b, then 3 x (w, b) Linear, then the LayerNorm g, b; zeros for absent biases) and packs
 * the images it reads from it on the device, so a call after an optimiser step sees the new weights with no host copy
 * and no synchronisation.  One plan serves one stream at a time.  npd_conv_train_destroy(NULL) is NPD_EINVAL.
 */
int npd_conv_train_create(int N, int embed, npd_conv_train** out);
int npd_conv_train_destroy(npd_conv_train* plan);
/*
 * Sizes (in floats) of the two caller-owned device buffers of a batch of B words (0 <= B <= 2^22), H = embed / 2:
 *   saved   (forward writes, backward reads): per conv layer the pre-activation z and the output, 2 B N (8 H + 2 embed);
 *           FC0 and FC1 z and output, 2 B (4 N + N); the dropout-scaled FC2 output, B N; the per-word mean and rstd,
 *           2 B rounded up to 4.
 *   scratch (backward's own): two gradient buffers of B N embed, two skip-gradient buffers of B N H, B N for the
 *           LayerNorm weight's per-word products, and the partial sums of the largest weight-gradient reduction (at
 *           most 2^26 floats: up to 4096 partials of a conv weight, about 1024 workgroups' worth of a Linear weight).
 * Both must be 16-byte aligned.  `saved` begins with, for conv layer i = 0 .. 9 in turn, z_i and then the layer's output
 * (after GELU and the residual), each (B, N, cout_i) with channels contiguous -- layer 5's output is convNet.forward's
 * input4; the rest of the layout is the library's.
 */
int npd_conv_train_workspace(const npd_conv_train* plan, int64_t B, int64_t* saved_floats, int64_t* scratch_floats);
/*
 * logits (B, N) = LayerNorm(drop_mult * FC2(...)), eps 1e-6.  y (B, N) device fp32, 16-byte aligned; drop_mult (B, N)
 * device fp32 of 0 or 1 / (1 - p), NULL = no dropout.  Launches on `stream`, no allocation, no synchronisation; words
 * beyond 32768 go to further launches of the conv kernels inside the call.  B = 0 returns NPD_OK with no launch.
 */
int npd_conv_train_forward(npd_conv_train* plan, const float* weights_dev, const float* y,
                           const float* drop_mult_or_null, float* logits, float* saved, int64_t B, void* stream);
/*
 * Backward of the forward that filled `saved` (same weights_dev, y, drop_mult, B): grad_weights_dev (flat, the weights'
 * order and length) is OVERWRITTEN with the gradient of sum(grad_logits * logits).  Every weight gradient is reduced
 * into per-workgroup partial sums that one kernel adds in a fixed order (no floating-point atomics: equal calls return
 * equal bits).  B = 0 zeroes the gradient.
 */
int npd_conv_train_backward(npd_conv_train* plan, const float* weights_dev, const float* y,
                            const float* drop_mult_or_null, const float* grad_logits, const float* saved, float* scratch,
                            float* grad_weights_dev, int64_t B, void* stream);

/* ---------------------------------------------------------------------------------- GPT transformer */
/*
 * XFormerEndToEndGPT.decode (models.py:398-423; run_models.py:338): at every information position i the whole
 * post-LN layer stack runs on tokens 0 .. i, each attending to every key <= i (mask row i), and
 * logit_i = Lin_Decoder(output of token i).  Token 0 = start_embed_layer(y); token j >= 1 = b_{j-1} pos_emb.weight[j],
 * b = +1 at a frozen position, sign(logit) at an information position.  fp32 throughout, dropout off.
 * Accepted: embed_dim 64, n_head 8, N = max_len in {16, 32, 64}, 1 <= n_layers <= 8; any information set.
 * weights: host fp32, the parameters decode reads, each row-major as in the state dict, in this order
 * (E = 64; n_weights = 192 N + 8449 + 49728 n_layers):
 *   start_embed_layer.0.weight (E,N), .0.bias (E), .2.weight (E,E), .2.bias (E), .4.weight (E,E), .4.bias (E),
 *   pos_emb.weight (N,E), Decoder.position_enc_auto.pos_table (N,E) -- the buffer's values, never recomputed --,
 *   then per layer l of Decoder.layer_stack: slf_attn.w_qs.weight (E,E), w_ks.weight, w_vs.weight, fc.weight,
 *   slf_attn.layer_norm.weight (E), .bias (E), pos_ffn.w_1.weight (4E,E), w_1.bias (4E), pos_ffn.w_2.weight (E,4E),
 *   w_2.bias (E), pos_ffn.layer_norm.weight (E), .bias (E),
 *   then Lin_Decoder.weight (E), Lin_Decoder.bias (1).
 */
typedef struct npd_gpt npd_gpt; /* a GPT decoder's weights, repacked for the kernel */
int npd_gpt_create(int N, int embed_dim, int n_head, int n_layers, const float* weights, int64_t n_weights,
                   npd_gpt** out);
/* a NULL handle is an argument error here (NPD_EINVAL), not a no-op */
int npd_gpt_destroy(npd_gpt* gpt);
/* scratch memory npd_gpt_decode takes from the caller: 0, the decode lives in LDS and registers (NPD_EINVAL for a
 * NULL handle or B < 0) */
int64_t npd_gpt_workspace_bytes(const npd_gpt* gpt, int64_t B);
/* y (B,N) device; is_info: N bytes of HOST memory, nonzero = information position (read before the call returns);
 * forced (B,N) device or NULL: token j is built from forced[:, j-1] instead of the decision; decoded (B,N) device:
 * sign(logit) at information positions (sign(0) = 0), +1 at frozen ones; logits (B,N) device or NULL: 0 at frozen
 * positions.  One launch on `stream`, no allocation; B = 0 returns NPD_OK. */
int npd_gpt_decode(const npd_gpt* gpt, const float* y, const uint8_t* is_info, const float* forced, float* decoded,
                   float* logits, int64_t B, void* stream);

/* ------------------------------------------------------------------- encoder / decoder transformer models */
/*
 * XFormerEndToEndDecoder.decode (models.py:635-654; --model decoder), with the attention mask applied to the keys of
 * every word (the masking branch under which the reference runs at any batch size).  Once per word the memory
 * Mem[j] = LN_cross(y_j emb_cross.weight[j+1] + position_enc_cross.pos_table[j]).  At every information position i
 * the layer stack runs on the tokens D[t] = LN(emb_inputs.weight[idx_t] + position_enc_auto.pos_table[t]), t = 0 .. i
 * (idx_0 = 2; idx_t = 1 if the bit at position t-1 is +1, else 0; a frozen position's bit is +1): per layer
 * self-attention over the keys <= i, cross-attention over all N rows of Mem, the FFN; logit_i = Lin_Decoder(token i).
 * Accepted: embed_dim 64, n_head 8, N = max_len in {16, 32, 64}, 1 <= n_layers <= 8; any information set.
 * weights: host fp32, each row-major as in the state dict, in this order (E = 64;
 * n_weights = 192 N + 641 + 66240 n_layers):
 *   Decoder.emb_cross.weight (N+1,E), Decoder.position_enc_cross.pos_table (N,E), Decoder.layer_norm_cross.weight (E),
 *   .bias (E), Decoder.emb_inputs.weight (4,E), Decoder.position_enc_auto.pos_table (N,E), Decoder.layer_norm.weight
 *   (E), .bias (E),
 *   then per layer l of Decoder.layer_stack: slf_attn.w_qs.weight (E,E), w_ks.weight, w_vs.weight, fc.weight,
 *   slf_attn.layer_norm.weight (E), .bias (E), the same six of enc_attn, pos_ffn.w_1.weight (4E,E), w_1.bias (4E),
 *   pos_ffn.w_2.weight (E,4E), w_2.bias (E), pos_ffn.layer_norm.weight (E), .bias (E),
 *   then Lin_Decoder.weight (E), Lin_Decoder.bias (1).
 * Both sinusoid tables are the buffers' values, never recomputed.
 */
typedef struct npd_xfdec npd_xfdec; /* a decoder model's weights, repacked for the kernel */
int npd_xfdec_create(int N, int embed_dim, int n_head, int n_layers, const float* weights, int64_t n_weights,
                     npd_xfdec** out);
/* a NULL handle is an argument error here (NPD_EINVAL), not a no-op */
int npd_xfdec_destroy(npd_xfdec* dec);
/* scratch memory npd_xfdec_decode takes from the caller: 0 (NPD_EINVAL for a NULL handle or B < 0) */
int64_t npd_xfdec_workspace_bytes(const npd_xfdec* dec, int64_t B);
/* the operands of npd_gpt_decode: y (B,N) device; is_info: N bytes of HOST memory; forced (B,N) device of +-1 or NULL:
 * token j is built from forced[:, j-1] instead of the decision; decoded (B,N) device; logits (B,N) device or NULL:
 * 0 at frozen positions.  One launch on `stream`, no allocation; B = 0 returns NPD_OK. */
int npd_xfdec_decode(const npd_xfdec* dec, const float* y, const uint8_t* is_info, const float* forced, float* decoded,
                     float* logits, int64_t B, void* stream);

/*
 * XFormerEndToEndEncoder.forward / decode (models.py:671-686; --model encoder) with an all-ones mask: one pass,
 * X[j] = LN(y_j Encoder.pos_emb.weight[j+1] + Encoder.position_enc.pos_table[j]), n_layers encoder layers with full
 * attention over the N tokens, logit[j] = Lin_Decoder(X[j]) for every j.  Accepted shapes as above.
 * weights, in this order (n_weights = 128 N + 257 + 49728 n_layers):
 *   Encoder.pos_emb.weight (N+1,E), Encoder.position_enc.pos_table (N,E), Encoder.layer_norm.weight (E), .bias (E),
 *   then per layer of Encoder.layer_stack the twelve tensors npd_gpt_create reads per layer,
 *   then Lin_Decoder.weight (E), Lin_Decoder.bias (1).
 */
typedef struct npd_xfenc npd_xfenc; /* an encoder model's weights, repacked for the kernel */
int npd_xfenc_create(int N, int embed_dim, int n_head, int n_layers, const float* weights, int64_t n_weights,
                     npd_xfenc** out);
int npd_xfenc_destroy(npd_xfenc* enc);                               /* NULL handle: NPD_EINVAL */
int64_t npd_xfenc_workspace_bytes(const npd_xfenc* enc, int64_t B); /* 0; NULL handle or B < 0: NPD_EINVAL */
/* y (B,N) device; bits (B,N) device: sign(logit) at every position (sign(0) = 0); logits (B,N) device or NULL.
 * One launch on `stream`, no allocation; B = 0 returns NPD_OK. */
int npd_xfenc_forward(const npd_xfenc* enc, const float* y, float* bits, float* logits, int64_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NPD_H_ */
