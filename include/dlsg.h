/* dlsg.h -- C ABI of libdlsg_hip.so: the MI355X (gfx950) kernels under the D-LSG CapGnnModel hot path.
 *
 * The reference (baiyang4/D-LSG-Video-Caption) has no native layer: every device op is a stock torch.nn call.
 * Each entry point below replaces the stock op(s) at the cited reference location.  All pointers are device
 * pointers owned by the caller; the library allocates nothing, keeps no global state, launches asynchronously
 * on `stream` (a hipStream_t passed as void*) and returns 0 or a negative DLSG_E* code.  All tensors are dense
 * fp32 row-major unless a leading dimension is given; ids are int64.
 *
 * Host-side bindings: d-lsg-video-caption_amd/dlsg_amd/hip.py (ctypes).  It does not repeat this file: dlsg_amd/abi.py reads it
 * when the package is imported and builds every argument struct, every prototype and the DLSG_* constants from the text below.
 * So this header stays in the subset of C that module knows, and it refuses anything else by line number: integer #defines;
 * `typedef struct { ... } dlsg_x;` whose members are fixed-width scalars, pointers, earlier structs by value and arrays of these;
 * prototypes that return int or int64_t.  See INTEGRATION.md.
 */
#ifndef DLSG_H
#define DLSG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever the signature or the meaning of an existing entry point changes (2: dlsg_colsum / dlsg_colsum2 take a
 * workspace pointer before the stream; the RCCL communicator entry points and the persistent BiLSTM were added).  A binding
 * must refuse a library whose version differs from the header it was written against.  (4: the critic's per-op entry points --
 * dlsg_lstm_cell_*, dlsg_tanh_ln_*, dlsg_conv_taps, dlsg_softmax_bwd2, dlsg_gemm_narrow -- gave way to the blocks of its schedule,
 * dlsg_crit_* / dlsg_cln_*; dlsg_lstm_seq takes batch-major arrays.  5: dlsg_gemm_args carries a workspace and an error word for the
 * stream-K kernel, dlsg_gemm_ws_bytes added; dlsg_adam takes `guard` before the stream and dlsg_select_embed `prefilled`.
 * 6: dlsg_gemm_args.err reserved, the stream-K kernel no longer waits.  7: dlsg_dec_tail_args samples the next word in the launch
 * (`s_*`), dlsg_o2v_bwd_args.dysum.  8: dlsg_gemm_args.cu_budget (was padding), dlsg_comm_rehearsal.) */
#define DLSG_ABI_VERSION 8
int dlsg_abi_version(void);

/* Return codes of every entry point that returns int: 0 or one of these. */
#define DLSG_OK 0
#define DLSG_EINVAL (-1)  /* an argument is out of the supported range (shape, count, NULL where data is required) */
#define DLSG_ELAUNCH (-2) /* the HIP runtime refused the launch / an RCCL call failed */
#define DLSG_EALIGN (-3)  /* a pointer or leading dimension misses the alignment the vector loads need */
#define DLSG_ENOCOMM (-4) /* librccl could not be loaded or the communicator handle is invalid */
/* sizeof() of the argument struct with index `which`, -1 for an index no struct has: lets a binding verify its struct layout
 * without a GPU.  The indices are in the order the structs were added, not the order of this file; the switch in
 * csrc/attention.hip is the list (a new struct gets the next index there). */
int dlsg_struct_size(int which);

/* ---------------------------------------------------------------- GEMM (fp32-in / fp32-acc MFMA 32x32x2)
 * Replaces every nn.Linear / LSTM gate matmul / torch.matmul on the path and their backward products:
 *   obj_embed layer.py:184, visual_embed :179, linear_embed :51, nn.LSTM :52, SelfAttention K/Q/V/out
 *   sublayer.py:66-68,80, AttentionShare K/V/Q/out sublayer.py:29-31,41, LSTMCell layer.py:571,593,
 *   word_restore layer.py:600.
 * C_g[b] (M x N, ldc) = alpha * opA(A_g[b]) . opB(B_g[b])  (+ bias[n]) (+ C) (tanh)   for every group g, batch b
 *   mode DLSG_GEMM_NT: A[m*lda+k], B[n*ldb+k]      (y = x W^T, Linear forward)
 *   mode DLSG_GEMM_NN: A[m*lda+k], B[k*ldb+n]      (dx = dy W)
 *   mode DLSG_GEMM_TN: A[k*lda+m], B[k*ldb+n]      (dW = dy^T x)
 * Groups share M, N, mode and flags but have their own operands, K and output: a K-split or a sum of several
 * (activation, weight) segments is expressed as groups writing separate slabs that the consumer kernel sums.
 */
#define DLSG_GEMM_NT 0 /* dlsg_gemm_args.mode */
#define DLSG_GEMM_NN 1
#define DLSG_GEMM_TN 2
#define DLSG_GEMM_MAXG 16
#define DLSG_GEMM_ACCUM 1 /* C += result */
#define DLSG_GEMM_BIAS 2  /* + bias[n]   */
#define DLSG_GEMM_TANH 4  /* tanh(.)     */
#define DLSG_GEMM_FORCE64 256  /* tuning: force the 64x64 block tile  */
#define DLSG_GEMM_FORCE128 512 /* tuning: force the 128x128 block tile (both FORCE bits: the 128x64 tile) */
#define DLSG_GEMM_TILE256 2048  /* tuning: force the 256x256 block tile of csrc/gemm_big.hip (with FORCE128: 256x128); EINVAL when
                                   the operands do not meet its alignment conditions */
#define DLSG_GEMM_SK 4096      /* tuning: force the persistent stream-K kernel of csrc/gemm_sk.hip; EINVAL without a workspace
                                  or when the operands do not meet its conditions (16-B alignment, K % 32 == 0, one batch) */
#define DLSG_GEMM_NOSK 8192    /* tuning: never the stream-K kernel */
#define DLSG_GEMM_SK_BM128 16384 /* tuning: the stream-K kernel on 128 x 256 tiles */
#define DLSG_GEMM_SK_BM256 32768 /* tuning: the stream-K kernel on 256 x 256 tiles */
#define DLSG_GEMM_SK_BN128 262144 /* tuning: the stream-K kernel on 128 x 128 tiles (shares half the size of the 128 x 256 tile's) */
#define DLSG_GEMM_SK_NOXMAP 131072 /* tuning: the stream-K kernel keeps all contributors of a tile on one XCD (no K-slice per XCD map) */
#define DLSG_GEMM_SK_GIVEAWAY 65536 /* test hook: no contributor of a split tile finds it complete -- every one gives its
                                       sub-blocks to the contributor that decides last (the path a launch that is not
                                       co-resident takes); same result bit for bit */
#define DLSG_GEMM_BF16X3 1024  /* split-bf16 matrix path: x = hi + lo, 3 bf16 MFMAs per product, fp32 accumulate
                                  (~1e-5 relative error per product instead of 6e-8; see csrc/gemm_bf16x3.hip) */
typedef struct {
    const float* A;
    const float* B;
    float* C;
    int64_t lda, ldb;
    int32_t K;
    int32_t N;   /* 0 = use args.N; otherwise this group's own output width (<= args.N): lets one launch write
                    column blocks of different widths (e.g. dG.W_ih and dG.W_hh) */
    const float* bias; /* optional per-group bias (overrides args.bias when DLSG_GEMM_BIAS is set) */
    int64_t ldc;       /* 0 = args.ldc; otherwise this group's own output row stride (groups writing into different arrays,
                          e.g. the weight-gradient blocks of one LSTM cell in one launch) */
} dlsg_gemm_group;
typedef struct {
    int32_t mode, M, N, ldc;
    int32_t ngroups, nbatch, flags;
    int32_t cu_budget;     /* 0 = the stream-K kernel launches one workgroup per CU; n > 0: at most n (rounded down to a multiple of
                              8), leaving the other CUs to a co-tenant -- a collective's kernels on another stream.  A stream-K
                              workgroup needs a whole CU, so without the budget its last workgroups would start only when the
                              first ones leave.  The tiled kernels ignore it */
    int64_t bsa, bsb, bsc; /* batch strides in elements */
    float alpha;
    int32_t pad2_;
    const float* bias;
    const int32_t* skip_if; /* optional device flag: the launch does nothing when *skip_if != 0 (a hipGraph-replayed step whose
                               product is needed only on some replays, e.g. per-word logits under scheduled sampling) */
    void* ws;               /* optional caller scratch of >= dlsg_gemm_ws_bytes() bytes, 16-B aligned, zero-filled ONCE by the
                               caller and not shared by launches that may run concurrently (one per stream): with it the
                               chip-filling products run on the persistent stream-K kernel (csrc/gemm_sk.hip), which leaves
                               the counter area at the front of it zeroed again; NULL = the tiled kernels only */
    int64_t ws_bytes;
    int32_t* err;           /* reserved (NULL): the stream-K kernel has no inter-workgroup wait that could time out -- the
                               contributor that completes a split tile adds the shares up */
    dlsg_gemm_group g[DLSG_GEMM_MAXG];
} dlsg_gemm_args;
int dlsg_gemm(const dlsg_gemm_args* args, void* stream);
/* Scratch a stream-K launch needs on the current device: a 16-KB counter area + two 256-KB accumulator slots per CU. */
int64_t dlsg_gemm_ws_bytes(void);
/* The kernel family dlsg_gemm runs this call on (fp32 arithmetic; EINVAL with DLSG_GEMM_BF16X3): what a profiler's kernel
 * symbol will be, without repeating the dispatch rule on the caller's side. */
#define DLSG_GEMM_V_64 0        /* gemm_kernel<64, 64, ...> */
#define DLSG_GEMM_V_128x64 1    /* gemm_kernel_w3<128, 64, ...> */
#define DLSG_GEMM_V_128 2       /* gemm_kernel_w3<128, 128, ...> */
#define DLSG_GEMM_V_SKINNY 3    /* skinny_kernel / skinny2_nt_kernel (M <= 128) */
#define DLSG_GEMM_V_256 4       /* gemm_big_kernel<256, 256, ...> */
#define DLSG_GEMM_V_256x128 5   /* gemm_big_kernel<256, 128, ...> */
#define DLSG_GEMM_V_256_HEAD 6  /* gemm_big_kernel<256, 256, ...> on the row panels that come in whole rounds of the CUs, the
                                   remaining rows through the choice again */
#define DLSG_GEMM_V_SK 7        /* gemm_sk_kernel<...>: one persistent launch, 256 x 256 tiles, stream-K remainder */
int dlsg_gemm_variant(const dlsg_gemm_args* args);

/* out[r, :] = sum_s slabs[s][r, :] (+ bias) (tanh); slabs are nslab consecutive (rows x n) arrays. */
int dlsg_slab_reduce(const float* slabs, int nslab, int64_t slab_stride, const float* bias, float* out,
                     int64_t rows, int n, int ldo, int flags, void* stream);

/* ---------------------------------------------------------------- row kernels: (tanh) -> LayerNorm -> (tanh) (+pe) (dropout)
 * Replaces nn.Sequential(Tanh, LayerNorm[, Dropout]) at layer.py:145-163, sublayer.py:183-187,21-26, and
 * the bare LayerNorms at layer.py:53,57,574,599 (+ PositionalEncoding_old add sublayer.py:102-104).
 *   z = x (+ res);  t = pre_tanh ? tanh(z) : z;  y = LN(t)*gamma+beta;  y = post_tanh ? tanh(y) : y;
 *   y = drop1(y);  if pe: y = drop2(y + pe[row % pe_rows]).   stats[row] = {mean, rstd}.
 */
typedef struct {
    const float* x; int64_t ldx;
    const float* res; int64_t ldres;      /* optional residual (NULL = none) */
    const float* gamma; const float* beta;
    float* y; int64_t ldy;
    float* stats;                          /* rows x 2, optional */
    const float* pe; int32_t pe_rows;     /* optional positional table (pe_rows x n) */
    int32_t rows, n;
    int32_t pre_tanh, post_tanh;
    float eps;
    float p1, p2;                          /* dropout probs (0 = off) */
    uint64_t seed; uint32_t site1, site2;
    const uint64_t* seed_ptr;              /* optional device word added to `seed` (graph replay: new masks per replay) */
} dlsg_rowln_args;
int dlsg_rowln_fwd(const dlsg_rowln_args* a, void* stream);
/* `count` (<= DLSG_ROWLN_MAXMULTI) norms of the same number of rows in one launch (the two encoder streams' visual_norm /
 * obj_visual_norm: 1 664 rows each put half the chip to work) */
#define DLSG_ROWLN_MAXMULTI 2
int dlsg_rowln_fwd_multi(const dlsg_rowln_args* a, int count, void* stream);
/* backward: dy -> dx (same shape as x; residual gets the same gradient), dgamma/dbeta partial sums are written
 * to dgb_part (nblk x 2 x n) and folded by dlsg_colsum. */
typedef struct {
    dlsg_rowln_args f;                     /* same descriptor as forward (y unused) */
    const float* dy; int64_t lddy;
    float* dx; int64_t lddx;
    int32_t accum_dx;                      /* dx += instead of = */
    float* dgb_part; int32_t nblk;         /* workspace: nblk x 2 x n ; nblk = grid size used */
} dlsg_rowln_bwd_args;
int dlsg_rowln_bwd(const dlsg_rowln_bwd_args* a, void* stream);
int dlsg_rowln_bwd_multi(const dlsg_rowln_bwd_args* a, int count, void* stream);
int dlsg_rowln_bwd_nblk(int rows);
/* out[j] (+)= sum_r part[r*ld + j], r < rows.  Tall inputs (rows >= 4096, e.g. the 26 624-row bias gradient of the region
 * projection) are summed in row chunks: with ws (>= dlsg_colsum_ws_floats(rows, n) floats of caller scratch) the chunk
 * partials are combined in a fixed order (bit-reproducible), with ws == NULL by float atomics. */
int64_t dlsg_colsum_ws_floats(int rows, int n);
int dlsg_colsum(const float* part, int64_t ld, int rows, int n, float* out, int accum, float* ws, void* stream);
/* two destinations in one pass: dup == 0 -> columns [0,split) to out_a, [split,n) to out_b (gamma | beta halves of the
 * LayerNorm partials); dup != 0 -> all n columns to both (bias_ih / bias_hh of an LSTM receive the same gradient). */
int dlsg_colsum2(const float* part, int64_t ld, int rows, int n, float* out_a, float* out_b, int split, int dup, int accum,
                 float* ws, void* stream);
/* `count` (<= DLSG_COLSUM_MAXMULTI) short column sums in one launch: each descriptor is one dlsg_colsum (out_b NULL) or
 * dlsg_colsum2 (out_b set; dup != 0: every column to both destinations, else columns [0, split) to out_a and the rest to out_b).
 * Only inputs dlsg_colsum_multi_ok() accepts (fewer than 4096 rows, 16-byte aligned, n and ld multiples of 4); no two descriptors of
 * one call may write the same destination.  Same additions in the same order as the single launches. */
#define DLSG_COLSUM_MAXMULTI 32
typedef struct {
    const float* part; int64_t ld;
    float* out_a; float* out_b;
    int32_t rows, n, split, dup, accum, pad_;
} dlsg_colsum_desc;
int dlsg_colsum_multi_ok(const float* part, int64_t ld, int rows, int n);
int dlsg_colsum_multi(const dlsg_colsum_desc* d, int count, void* stream);

/* ---------------------------------------------------------------- object->frame conditional graph (layer.py:184-193)
 * y (B, NO, H) = tanh(obj_embed(regions)) (the GEMM epilogue applied tanh); LayerNorm(obj_norm) is applied on the
 * fly.  v (B, T, H) = visual_norm output.  Computes
 *   S[n,t] = LN(y_n).v_t / sqrt(obj_size);  P = softmax over n;  agg_t = sum_n P[n,t] LN(y_n);  z = agg + v
 * Partial kernel: grid (B, nsplit) online-softmax over an object chunk; combine merges chunks, writes z (pre
 * obj_visual_norm), the softmax statistics m,l (B,T) and the object LN stats (B*NO x 2).
 */
typedef struct {
    const float* y; const float* v;
    const float* g_obj; const float* b_obj;     /* obj_norm.1 weight/bias */
    float* z;                                    /* (B,T,H) agg + v */
    float* ml;                                   /* (B,T,2) softmax max / sum (of exp(S-max)) */
    float* ostats;                               /* (B*NO,2) LN mean/rstd of y rows */
    float* S;                                    /* (B,NO,T) raw scaled scores, saved for backward */
    float* ws; int64_t ws_bytes;                 /* workspace for partials */
    int32_t B, T, NO, H, nsplit;
    float scale, eps;
} dlsg_o2v_args;
int64_t dlsg_o2v_workspace_bytes(int B, int T, int H, int nsplit);
int dlsg_o2v_fwd(const dlsg_o2v_args* a, void* stream);
/* `count` (<= DLSG_O2V_MAXMULTI) graphs of one shape (B, T, NO, H, nsplit equal) in one launch: CapGnnEncoder runs the same
 * graph on the object and the motion stream (models/model.py:69-73); together they fill the chip with half the object
 * chunks per clip.  a[0..count) are consecutive argument blocks. */
#define DLSG_O2V_MAXMULTI 2
int dlsg_o2v_fwd_multi(const dlsg_o2v_args* a, int count, void* stream);
/* Backward of the fused graph in two passes over y (csrc/o2v16_bwd.hip; one workgroup per (clip, object chunk, stream) on
 * the forward's LDS-DMA tile pipeline): given dz (B,T,H) it writes
 *   dy (B,NO,H)  grad wrt the obj_embed pre-activation (through obj_norm's LayerNorm and the tanh of the GEMM epilogue),
 *   dv (B,T,H)   grad wrt the frame nodes v (includes the residual dz),
 *   part (B*nsplit,2,H) dgamma | dbeta of obj_norm per (clip, object chunk) (fold with dlsg_colsum2),
 *   dysum (B*nsplit,H), optional: the column sums of dy per (clip, object chunk) -- obj_embed's bias gradient without another
 *                pass over the (B*NO)-row dy (fold with dlsg_colsum).
 * y, ostats, S, ml, z are the forward's inputs / outputs; pd (B,NO,64) and m12 (B,NO,2) are workspaces, ws = dlsg_o2v_workspace_bytes
 * (B, T, H, nsplit) bytes of chunk partials of dv (needed when nsplit > 1).  dlsg_o2v_bwd_multi: `count` (<= DLSG_O2V_MAXMULTI)
 * graphs of one shape in one launch per pass (the object and the motion stream of CapGnnEncoder).
 * Same support as the forward (T <= 32, H in {64,512,1024}); otherwise the caller runs the unfused chain
 * (dlsg_softmax_fwd/bwd on S + batched dlsg_gemm + dlsg_rowln_bwd; engine.py tun_bwd).
 */
typedef struct {
    const float* y; const float* ostats; const float* g_obj; const float* b_obj;
    const float* v; const float* z; const float* dz; const float* S; const float* ml;
    float* pd; float* m12;
    float* dy; float* dv; float* part;
    float* ws; int64_t ws_bytes;
    int32_t B, T, NO, H, nsplit;
    float scale;
    float* dysum;
} dlsg_o2v_bwd_args;
int dlsg_o2v_bwd_multi(const dlsg_o2v_bwd_args* a, int count, void* stream);
int dlsg_o2v_bwd(const dlsg_o2v_bwd_args* a, void* stream);

/* ---------------------------------------------------------------- LatentPSL forward (sublayer.py:189-198), one launch
 * adj (B,T,P) = softmax over the frames of ov . theta^T;  u (B*P,H) = adj^T ov;  out = Dropout(LayerNorm(tanh(u))).
 * T <= 32, P <= 32, H <= 2048 (multiple of 4), T*H*4 <= 140 KB of LDS; otherwise the caller runs the unfused chain
 * (2 x dlsg_gemm + dlsg_softmax_fwd + dlsg_rowln_fwd), which is also what the backward consumes (adj, u, stats). */
typedef struct {
    const float* ov; const float* theta; const float* gamma; const float* beta;
    float* adj; float* u; float* out; float* stats;
    int32_t B, T, P, H;
    float p; uint32_t site; float eps; float pad_;
    uint64_t seed; const uint64_t* seed_ptr;
} dlsg_latent_psl_args;
int dlsg_latent_psl_fwd(const dlsg_latent_psl_args* a, void* stream);
/* `count` (<= DLSG_PSL_MAXMULTI) LatentPSL modules of one shape (B, P, H equal) in one launch: CapGnnEncoder's object and
 * motion stream (one workgroup per clip: 64 clips alone leave three quarters of the chip idle) */
#define DLSG_PSL_MAXMULTI 2
int dlsg_latent_psl_fwd_multi(const dlsg_latent_psl_args* a, int count, void* stream);
/* backward (P <= 8, (T+8)*H*4 <= 150 KB of LDS): dout (B*P,H) -> dov (B*T,H) written, dtheta_part (B,P,H) and
 * part (B,2,H) = per-clip partials of dtheta and of out_norm's dgamma | dbeta (fold with dlsg_colsum / dlsg_colsum2).
 * u, stats, adj are the forward's outputs; p/site/seed the forward's dropout. */
typedef struct {
    const float* dout; const float* u; const float* stats; const float* gamma;
    const float* adj; const float* ov; const float* theta;
    float* dov; float* dtheta_part; float* part;
    int32_t B, T, P, H;
    float p; uint32_t site;
    uint64_t seed; const uint64_t* seed_ptr;
} dlsg_latent_psl_bwd_args;
int dlsg_latent_psl_bwd(const dlsg_latent_psl_bwd_args* a, void* stream);
int dlsg_latent_psl_bwd_multi(const dlsg_latent_psl_bwd_args* a, int count, void* stream);

/* ---------------------------------------------------------------- SelfAttention 26x26 core (sublayer.py:69-78), one launch
 * w (B,T,T) = softmax_j(K_i . Q_j * scale) (optional mask (B,T,T): mask <= 0 -> -9e15 as sublayer.py:70-72);
 * out (B,T,D) = w V.  T <= 32, D a multiple of 64; otherwise dlsg_gemm + dlsg_softmax_fwd + dlsg_gemm. */
typedef struct {
    const float* K; const float* Q; const float* V; const float* mask;
    float* w; float* out;
    int32_t B, T, D; float scale;
} dlsg_sa_core_args;
int dlsg_sa_core_fwd(const dlsg_sa_core_args* a, void* stream);
/* backward of the core: dout (B,T,D) and the saved w -> dK, dQ, dV (B,T,D), all dense (row stride D). */
typedef struct {
    const float* w; const float* K; const float* Q; const float* V; const float* dout;
    float* dK; float* dQ; float* dV;
    int32_t B, T, D; float scale;
} dlsg_sa_core_bwd_args;
int dlsg_sa_core_bwd(const dlsg_sa_core_bwd_args* a, void* stream);

/* ---------------------------------------------------------------- softmax along the middle axis of (outer, n, inner)
 * LatentPSL softmax over frames (sublayer.py:192: outer=B, n=T, inner=P), SelfAttention row softmax
 * (sublayer.py:74: inner=1, optional mask: mask<=0 -> -9e15 as sublayer.py:70-72), o2v softmax over objects
 * (layer.py:188: n=T*O, inner=T).  The dense products around them run through dlsg_gemm (batched). */
int dlsg_softmax_fwd(const float* x, const float* mask, float* y, int64_t outer, int n, int inner, void* stream);
/* dx = y * (dy - sum_n y*dy) */
int dlsg_softmax_bwd(const float* y, const float* dy, float* dx, int64_t outer, int n, int inner, void* stream);

/* ---------------------------------------------------------------- decoder attention over cached K', V' (sublayer.py:28-43)
 * For stream s in {0,1}: score_p = K'_s[b,p,:].q[b,:] * scale; w = softmax over p; c = sum_p w_p V'_s[b,p,:].
 * K' = (m W_K^T) W_Q and V' = (m W_V^T) W_O^T are precomputed once per forward (step-invariant), so the per-step
 * work is this kernel only.  Writes c (pre tanh/LN) and alpha (B, 2P). */
typedef struct {
    const float* Kp[2]; const float* Vp[2];   /* (B,P,Q) and (B,P,H) */
    const float* q; int64_t ldq;              /* (B,Q) */
    float* c[2]; int64_t ldc;                 /* (B,H) each */
    float* alpha;                             /* (B, nstream*P) */
    int32_t B, P, Q, H, nstream;
    float scale;
} dlsg_decatt_args;
int dlsg_decatt_fwd(const dlsg_decatt_args* a, void* stream);
typedef struct {
    dlsg_decatt_args f;
    const float* dc[2]; int64_t lddc;         /* (B,H) */
    const float* dalpha;                      /* optional (B, nstream*P) */
    float* dKp[2]; float* dVp[2];             /* accumulated (+=) over steps */
    float* dq; int64_t lddq; int32_t accum_dq;
} dlsg_decatt_bwd_args;
int dlsg_decatt_bwd(const dlsg_decatt_bwd_args* a, void* stream);

/* ---------------------------------------------------------------- fused decoder step (Decoder.decode, layer.py:569-602)
 * One workgroup per batch row; everything between the two gate GEMMs of a word step in ONE launch:
 *   query LSTM cell pointwise (sums the gate GEMM's slabs) -> query_lstm_layernorm (+dropout) -> attention over the
 *   cached K', V' of every stream (scores, softmax over P, weighted V') -> tanh -> output_layer LayerNorm (+dropout).
 * Replaces dlsg_lstm_pw_fwd + dlsg_rowln_fwd + dlsg_decatt_fwd + 2 x dlsg_rowln_fwd of the unfused schedule. */
typedef struct {
    /* query cell */
    const float* slabs; int32_t nslab; int32_t pad_; int64_t slab_stride;     /* (S,B,4Q) gate partial sums */
    const float* addend; int64_t ldadd;          /* (B,4Q) global-feature gate part */
    const float* b_ih; const float* b_hh;
    const float* c_prev;                         /* (B,Q) */
    float* c; float* h; float* gates;            /* (B,Q), (B,Q) raw h, (B,4Q) activated gates */
    const float* lnq_g; const float* lnq_b;      /* query_lstm_layernorm */
    float* qcur; float* st_q;                    /* (B,Q) dropout(LN(h)), (B,2) */
    float p_q; uint32_t site_q;
    /* attention streams */
    const float* Kp[2]; const float* Vp[2];      /* (B,P,Q), (B,P,H) */
    const float* lnc_g[2]; const float* lnc_b[2];/* output_layer.2 of each AttentionShare */
    float* cpre[2]; float* ctx[2]; float* st_c[2];   /* (B,H) pre-tanh context, (B,H) output, (B,2) */
    float* alpha;                                /* (B, nstream*P) */
    float p_att[2]; uint32_t site_att[2];
    int32_t B, Q, H, P, nstream;
    float scale, eps;
    int32_t kv_div;                              /* <= 1: row b attends over K'[b], V'[b].  k > 1 (beam search: the k beams of a
                                                    clip are consecutive rows): row b attends over K'[b / k], V'[b / k], which
                                                    then hold one block per CLIP -- the beams share the lines in L2 instead of
                                                    each streaming its own expanded copy */
    uint64_t seed; const uint64_t* seed_ptr;
    int32_t sched;                               /* 0: the library's choice (early loads when B <= the device's CUs, so that the
                                                    workgroup has its CU's registers to itself); 1: loads requested where they
                                                    are used; 2: every load whose address depends on nothing the kernel computes
                                                    requested up front into registers.  Same arithmetic, bit-identical outputs */
} dlsg_dec_mid_args;
int dlsg_dec_mid_fwd(const dlsg_dec_mid_args* a, void* stream);
/* language LSTM cell pointwise (+dropout on h) -> tanh(lang_lstm_layernorm(h)) for the vocab projection. */
typedef struct {
    const float* slabs; int32_t nslab; int32_t pad_; int64_t slab_stride;     /* (S,B,4D) */
    const float* b_ih; const float* b_hh;
    const float* c_prev; float* c; float* hd; float* gates;    /* (B,D) ..., hd = dropout(h) (next state), (B,4D) */
    const float* ln_g; const float* ln_b;
    float* dout; float* st_l;                   /* (B,D) tanh(LN(hd)), (B,2) */
    float p; uint32_t site;
    int32_t B, D;
    float eps;
    uint64_t seed; const uint64_t* seed_ptr;
    /* optional (s_coins != NULL): scheduled sampling of the NEXT step's word inside this launch (models/layer.py:432-441).  When
     * s_coins[s_t] == 0 every workgroup projects its row onto the vocabulary (s_W (V x D), s_b), takes the first maximum, writes
     * it to s_ids[b] and its embedding row (s_E (V x W), word dropout s_p / s_site at row s_row0 + b, the mask stream of
     * dlsg_embed_fwd / dlsg_select_embed) to s_we; when the coin is set (teacher-forced step, ids and embedding filled in up
     * front) nothing more happens.  One weight read per workgroup: for vocabularies up to ~2 M weights; larger ones keep
     * dlsg_gemm + dlsg_select_embed.  Replaces two launches per word step that do nothing on ~19 steps out of 20. */
    const int32_t* s_coins; int32_t s_t; int32_t s_V;
    const float* s_W; const float* s_b;
    const float* s_E; int32_t s_Wd; uint32_t s_site;
    int64_t* s_ids; float* s_we; int64_t s_ldwe;
    int64_t s_row0; float s_p; float pad2_;
    /* optional (s_ws != NULL): the vocabulary scan of a sampled step split over S workgroups per row, grid B x S, still one launch.
     * Part 0 of a row is the workgroup described above; on a sampled step it scans only the first of S contiguous shares of the
     * vocabulary.  Parts 1 .. S-1 read the coin first and return on a teacher-forced step; on a sampled step they recompute the
     * row's dout (same arithmetic, no stores) and scan their share.  Every part leaves its (best logit, first index) in the
     * row's workspace and draws a ticket from the row's counter; the part that draws the last one takes the maximum of the S
     * pairs (lower index on equality), writes s_ids / s_we and sets the counter back to 0.  No part waits for another, and
     * every output has the bits of the unsplit launch.
     * s_ws: DLSG_DEC_TAIL_WS_WORDS int32 words per row, 8-byte aligned, ZEROED ONCE by the caller when it is allocated and never
     * again (every sampled launch leaves the counters at 0; a teacher-forced one does not touch them); not shared by two
     * launches that may run at the same time.  s_split: 0 the library's choice, dlsg_dec_tail_split(B, CUs of the device);
     * 1 unsplit; 2 .. DLSG_DEC_TAIL_MAX_SPLIT forced (tests).  Unsplit as well when s_ws or s_coins is NULL or c_prev == c
     * (the other parts would read what part 0 writes).  Zeroed fields: the launch of ABI 7. */
    int32_t* s_ws; int32_t s_split; int32_t pad3_;
} dlsg_dec_tail_args;
#define DLSG_DEC_TAIL_MAX_SPLIT 8
#define DLSG_DEC_TAIL_WS_WORDS 32 /* per row: MAX_SPLIT 8-byte pairs, the ticket counter, padding to one 128-byte line */
int dlsg_dec_tail_fwd(const dlsg_dec_tail_args* a, void* stream);
/* host only, no launch: the split dlsg_dec_tail_fwd chooses for s_split = 0 on a device of `cus` compute units --
 * min(DLSG_DEC_TAIL_MAX_SPLIT, cus / B), at least 1: the parts of all rows fit the device together. */
int dlsg_dec_tail_split(int32_t B, int32_t cus);
/* Backward of dlsg_dec_mid_fwd for one word step, one workgroup per batch row.  Consumes the slabs of the language
 * cell's input-gradient GEMM directly (their sum is [d ctx_0 | d ctx_1 | d q_cur | d lang_h(recurrent)]), runs the
 * output_layer LayerNorm backward of each stream, the attention backward (score / softmax / context), the
 * query_lstm_layernorm backward and the query cell backward.  The gradients of the cached K', V' are NOT accumulated
 * here: the step leaves d(pre-tanh context) and d(score) in per-step buffers and dlsg_decatt_cache_grads contracts them
 * over the word loop afterwards (no read-modify-write of the (B,P,Q)+(B,P,H) caches per word).
 * Replaces dlsg_slab_reduce + 2 x dlsg_rowln_bwd + dlsg_decatt_bwd + dlsg_rowln_bwd + dlsg_lstm_pw_bwd. */
typedef struct {
    const float* slabs; int32_t nslab; int32_t write_rec; int64_t slab_stride;   /* (S,B,ns*H+Q+D), rows dense */
    float* dlh_rec;                      /* (B,D) out when write_rec: sum of the last D columns */
    const float* cpre[2]; const float* st_c[2]; const float* lnc_g[2];
    float* part_c[2];                    /* (B,2,H) per-row dgamma | dbeta of each output_layer LayerNorm */
    float* dcpre[2];                     /* (B,H) out */
    float p_att[2]; uint32_t site_att[2];
    const float* Kp[2]; const float* Vp[2];
    const float* alpha; const float* dalpha;     /* (B,ns*P); dalpha optional */
    float* ds;                           /* (B,ns*P) out */
    const float* qh; const float* st_q; const float* lnq_g;
    float* part_q;                       /* (B,2,Q) */
    float p_q; uint32_t site_q;
    const float* rec_slabs; int32_t rec_nslab; int32_t pad_; int64_t rec_slab_stride; int64_t rec_ld;
                                         /* (S',B,>=Q): recurrent d h_query from step t+1, NULL at the last step */
    const float* gates; const float* c; const float* c_prev;   /* (B,4Q), (B,Q), (B,Q) */
    float* dc;                           /* (B,Q) in/out: cell-state gradient */
    float* dgates;                       /* (B,4Q) out */
    int32_t B, Q, H, D, P, nstream;
    float scale; float pad2_;
    uint64_t seed; const uint64_t* seed_ptr;
    int32_t sched;                       /* as dlsg_dec_mid_args.sched */
} dlsg_dec_mid_bwd_args;
int dlsg_dec_mid_bwd(const dlsg_dec_mid_bwd_args* a, void* stream);
/* dK'[s][b,p,:] = sum_t ds[t,b,s*P+p] * q_cur[t,b,:],  dV'[s][b,p,:] = sum_t alpha[t,b,s*P+p] * dcpre[s][t,b,:]
 * (time-major (L,B,.) inputs; outputs written, not accumulated). */
typedef struct {
    const float* alpha; const float* ds;         /* (L,B,ns*P) */
    const float* qcur;                           /* (L,B,Q) */
    const float* dcpre[2];                       /* (L,B,H) */
    float* dKp[2]; float* dVp[2];                /* (B,P,Q), (B,P,H) */
    int32_t L, B, Q, H, P, nstream;
} dlsg_decatt_cache_grads_args;
int dlsg_decatt_cache_grads(const dlsg_decatt_cache_grads_args* a, void* stream);

/* ---------------------------------------------------------------- LSTM cell pointwise (nn.LSTM layer.py:52, nn.LSTMCell :571,593)
 * gates = sum_s slabs[s] (+ addend) (+ b_ih + b_hh), PyTorch gate order i,f,g,o;
 * c = f*c_prev + i*g; h = o*tanh(c).  Saves activated gates (B,4H) for backward.  h is written to up to two
 * destinations (strided); h2 receives dropout(h) when p>0 (lang_lstm_drop layer.py:594). */
typedef struct {
    const float* slabs; int32_t nslab; int32_t pad_; int64_t slab_stride;
    const float* addend; int64_t ldadd;        /* optional precomputed gate part (B,4H) */
    const float* b_ih; const float* b_hh;      /* optional */
    const float* c_prev; int64_t ldcp;         /* NULL = zeros */
    float* c; int64_t ldc_;
    float* h; int64_t ldh;                     /* raw h (recurrent state) */
    float* h2; int64_t ldh2;                   /* optional second copy (dropout applied if p>0) */
    float* gates; int64_t ldg;                 /* (B,4H) activated gates (row stride ldg), optional */
    int32_t B, H;
    float p; uint32_t site; uint64_t seed;
    const uint64_t* seed_ptr;
} dlsg_lstm_pw_args;
int dlsg_lstm_pw_fwd(const dlsg_lstm_pw_args* a, void* stream);
/* `count` (1 or 2) descriptors of equal B, H in one launch: the two directions of a BiLSTM step */
int dlsg_lstm_pw_fwd_n(const dlsg_lstm_pw_args* a, int count, void* stream);
/* backward: dh (B,H) [+ dh2 through dropout], dc_next -> dgates (B,4H pre-activation grads), dc_prev */
typedef struct {
    const float* gates; int64_t ldg;           /* activated gates from forward, row stride ldg */
    const float* c; int64_t ldc_;
    const float* c_prev; int64_t ldcp;
    const float* dh; int64_t lddh;             /* optional */
    const float* dh2; int64_t lddh2;           /* optional, goes through the dropout mask */
    const float* dh3; int64_t lddh3;           /* optional, summed with dh2 before the mask */
    const float* dh4; int64_t lddh4;           /* optional, summed with dh2 before the mask */
    int32_t dh4_nslab; int32_t pad4_; int64_t dh4_slab_stride;   /* dh4_nslab > 1: dh4 is a slab stack, summed on the fly */
    const float* dc_next; int64_t lddcn;       /* optional */
    float* dgates; int64_t lddg;               /* (B,4H) pre-activation gate grads, row stride lddg */
    float* dc_prev; int64_t lddcp;
    int32_t B, H;
    float p; uint32_t site; uint64_t seed;
    const uint64_t* seed_ptr;
} dlsg_lstm_pw_bwd_args;
int dlsg_lstm_pw_bwd(const dlsg_lstm_pw_bwd_args* a, void* stream);
int dlsg_lstm_pw_bwd_n(const dlsg_lstm_pw_bwd_args* a, int count, void* stream);

/* ---------------------------------------------------------------- small data movement on the path
 * mean over P proposals (layer.py:407-410): out[b, off + h] = mean_p x[b,p,h]; and its backward (accumulating) */
int dlsg_mean_rows_fwd(const float* x, float* out, int64_t ldo, int B, int P, int H, void* stream);
int dlsg_mean_rows_bwd(const float* dout, int64_t lddo, float* dx, int B, int P, int H, int accum, void* stream);
/* several captions per clip on one encoder pass: y[b*n + i, :] = x[b, :] for i < n (x: B contiguous rows of `row` floats, y: B*n);
 * 16-byte accesses when row % 4 == 0 and both bases are 16-byte aligned, else a scalar path */
int dlsg_rows_repeat(const float* x, float* y, int B, int n, int64_t row, void* stream);
/* and the fold of the caption rows' gradients back onto the clip, with the backward of the proposals' mean in the same pass:
 * dx[b,p,h] (+)= sum_{i<n} (dmem[b*n + i, p, h] + dg[(b*n + i)*lddg + h] / P), added in the order i = 0..n-1 by one thread per
 * output element (no atomics: bit-reproducible).  dmem (B*n,P,H) and dx (B,P,H) contiguous; dg optional (NULL: no mean term),
 * B*n rows of H floats with row stride lddg >= H; accum != 0 adds to dx. */
int dlsg_clip_fold(const float* dmem, const float* dg, int64_t lddg, float* dx, int B, int n, int P, int H, int accum, void* stream);
/* embedding gather + dropout (layer.py:421-422,438-439): out[r, :] = drop(E[ids[r], :]); the dropout mask of
 * element (r, j) is keyed by (row0 + r) * W + j so a slice of a larger call reproduces the same mask. */
int dlsg_embed_fwd(const float* E, const int64_t* ids, float* out, int64_t ldo, int rows, int W, float p, uint64_t seed,
                   uint32_t site, int64_t row0, const uint64_t* seed_ptr, void* stream);
/* dE[ids[r], :] += drop(dout[r, :])   (atomic adds; rows sharing an id collide) */
int dlsg_embed_bwd(const float* dout, int64_t lddo, const int64_t* ids, float* dE, int rows, int W, float p,
                   uint64_t seed, uint32_t site, int64_t row0, const uint64_t* seed_ptr, void* stream);
/* scheduled sampling on device (layer.py:432-439): id[b] = coins[t] ? captions[b*L + t] : argmax(logits[b, :]);
 * ids_out[b] = id; out[b, :] = drop(E[id, :]).  coins is a device int32 array, so a captured graph is invariant to the
 * coin pattern.  prefilled != 0: the caller wrote the teacher-forced choice of this step into ids_out / out up front (one
 * dlsg_embed_fwd over all steps), so the launch is a no-op when coins[t] is set. */
int dlsg_select_embed(const float* logits, int64_t ld, int V, const int64_t* captions, int L, int t, const int32_t* coins,
                      const float* E, int64_t* ids_out, float* out, int64_t ldo, int rows, int W, float p, uint64_t seed,
                      uint32_t site, int64_t row0, const uint64_t* seed_ptr, int prefilled, void* stream);
/* argmax over logits rows (first max wins, like torch.max) */
int dlsg_argmax(const float* logits, int64_t ld, int64_t* ids, int rows, int V, void* stream);
/* sampled decoding (self-critical training): ids_out[r] = a word drawn from softmax(logits[r, :] / temperature) by Gumbel-max,
 * argmax_j (x_j / temperature + g_j) with g_j = -log(-log u_j) and u_j from the dropout hash keyed (seed (+ *seed_ptr),
 * site_sample, (row0 + r) * V + j) -- stateless, so a replayed graph with the same seed draws the same words;
 * logp[r] = log softmax(logits[r, :] / temperature)[id]; out[r, :] = drop(E[id, :]) with the word-dropout mask of
 * dlsg_embed_fwd (seed, site_word, row0 + r); lens[r] (int64, set to L by the caller) becomes t + 1 when id == end_id and
 * lens[r] > t.  temperature 0: the id of dlsg_argmax (first maximum) and logp of the untempered softmax.  A row without a
 * maximum (all NaN / -inf) gives id 0; a -inf logit is never drawn.  E has at least V rows of W floats. */
int dlsg_sample_embed(const float* logits, int64_t ld, int V, float temperature, const float* E, int64_t* ids_out, float* out,
                      int64_t ldo, int W, float* logp, int64_t* lens, int t, int64_t end_id, int rows, float p, uint64_t seed,
                      uint32_t site_word, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, void* stream);
/* dlsg_sample_embed behind logits processors and warpers, in the order of the usual toolkits (processors, then warpers).  For
 * row r at word step t, z_j = logits[r, j] / temperature:
 *   1. bans (z_j = -inf): end_id while t < min_len; with g = no_repeat_ngram > 0, every class c for which an i <= t - g exists
 *      with h[i .. i+g-2] == h[t-g+1 .. t-1] and h[i+g-1] == c (the rule of dlsg_beam_select_hist on the row's own words:
 *      h[i] = hist[i * hist_stride + r], i < t, time-major ids; hist may be NULL when g == 0).  NaN and -inf logits are never kept;
 *   2. top_k (0 = off): keep {j : z_j >= v_k}, v_k the k-th largest unbanned value -- ties at v_k are all kept;
 *   3. top_p in (0, 1] (1 = off), over what top_k kept: theta = the largest value with mass{z_j >= theta} >= top_p * mass(kept
 *      by top_k) (mass = sum of exp(z_j - max), float32, summed in a fixed order), keep {z_j >= theta}: never empty;
 *   4. the draw: Gumbel-max over the kept set with the noise of dlsg_sample_embed, keyed (seed, site_sample, (row0 + r) * V + j)
 *      -- a word's noise does not depend on the filters, and the word drawn is the one dlsg_sample_embed draws from the same row
 *      with the logits that are not kept set to -inf;
 *   5. logp[r] = z_id - logsumexp(z over the kept set), the log-probability under the distribution drawn from (exactly 0 when
 *      one word is kept); kept[r] (may be NULL) = the size of the kept set; lens, out and the word dropout as dlsg_sample_embed.
 * temperature 0: the first maximum over the unbanned words, top_k and top_p ignored, logp of the untempered softmax over the
 * unbanned words, kept = their number.  A row with nothing to keep gives word 0 and kept 0.  No atomics and fixed reduction
 * orders: two launches, or a launch and a graph replay, give the same bits.  One workgroup per row stages the row in LDS:
 * 1 <= V <= DLSG_SAMPLE_FILTER_MAXV, a larger V returns DLSG_EINVAL (the row is not re-read from memory).  0 <= t < 64. */
#define DLSG_SAMPLE_FILTER_MAXV 32768
int dlsg_sample_filter_embed(const float* logits, int64_t ld, int V, float temperature, const float* E, int64_t* ids_out, float* out,
                             int64_t ldo, int W, float* logp, int64_t* lens, int t, int64_t end_id, int rows, float p, uint64_t seed,
                             uint32_t site_word, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, int top_k, float top_p,
                             int min_len, int no_repeat_ngram, const int64_t* hist, int64_t hist_stride, int32_t* kept, void* stream);
/* strided 2-d copy / add: dst[r*ldd + j] (+)= src[r*lds + j] */
int dlsg_copy2d(const float* src, int64_t lds, float* dst, int64_t ldd, int rows, int n, int accum, void* stream);
/* elementwise dropout with the stateless mask: y = x * keep(seed, site, r*n+j)/(1-p) */
int dlsg_dropout(const float* x, int64_t ldx, float* y, int64_t ldy, int rows, int n, float p, uint64_t seed,
                 uint32_t site, const uint64_t* seed_ptr, void* stream);
int dlsg_fill(float* dst, int64_t n, float value, void* stream);
/* dst[r, :] = src[idx[r], :]  (beam-search state reorder by back-pointer, allennlp_beamsearch.py:248-260) */
int dlsg_gather_rows(const float* src, int64_t lds, const int64_t* idx, float* dst, int64_t ldd, int rows, int n, void* stream);
/* dst[b,t,:] = src[t,b,:]: time-major decoder buffers -> the (B,L,V) layout Decoder.forward returns (layer.py:447) */
int dlsg_permute_tb(const float* src, float* dst, int T, int B, int n, void* stream);

/* ---------------------------------------------------------------- DiscV2 critic: the blocks of its schedule
 * `DiscV2.forward` (models/model.py:143-166), `PSLScore2.forward` (models/layer.py:690-715), `SelfAttention` with the caption mask
 * (models/sublayer.py:63-82), `LatentPSL` (sublayer.py:189-198), `ResBlock` (sublayer.py:107-119) and the WGAN-GP critic update
 * around them (run_gun.py:339-381: three critic forwards, gradient penalty with create_graph=True, loss backward) as explicit
 * passes of dlsg_amd/critic.py.  Every block exists at three levels:
 *   fwd   the block's forward;
 *   bwd   its vector-Jacobian product (inputs; parameters where it has any);
 *   bwd2  the DIRECTIONAL DERIVATIVE of (fwd, bwd) along a tangent U of the block's input at fixed output cotangent -- what the
 *         gradient penalty's second-order term needs of a block: the derivative of fwd is the tangent handed to the next block,
 *         the derivative of bwd's input gradient an extra cotangent on the block's input, the derivative of bwd's parameter
 *         gradient an extra parameter gradient.
 * Activations are batch-major: (captions, L words, 512) dense; `captions` = n blocks of B ("caption sets" scored against the same
 * B clips: caption i belongs to clip i % B).  acc_lo / acc_hi: a caption (or row) range whose outputs are ADDED to what the
 * buffer holds (the extra cotangents of the bwd2 pass) instead of written.  Dropout is the stateless mask of the generator path
 * (keyed by seed + *seed_ptr, site, element index); p = 0 switches it off.  L <= 32, T <= 8 proposals, width 512. */
#define DLSG_CRIT_C 512
#define DLSG_CRIT_LMAX 32
#define DLSG_CRIT_TMAX 8

/* Vocabulary projection glue (models/model.py:143-144 on one-hot / logit inputs, run_gun.py:447-451,358-360).
 * embed_mix: proj_tm (L,B,512) = logits W^T without bias; ids (B,L) or NULL; W (512,V); eps (B) or NULL.
 *   ng = 3: h[0] = W[:, ids] + bias (real captions as a gather of weight columns), h[1] = proj + bias, h[2] = eps h[0] + (1-eps) h[1];
 *   ng = 1: h[0] = proj + bias.   h (ng, B, L, 512).
 * embed_mix_bwd: ch (ng,B,L,512) -> dhr (B,L,512) = ch[0] + eps ch[2] and dhf_tm (L,B,512) = ch[1] + (1-eps) ch[2]  (ng = 1: dhf_tm = ch[0]^T).
 * vocab_scatter: dW[:, ids[b,l]] += dhr[b,l,:] in a fixed order (the first row carrying an id adds all rows of that id). */
int dlsg_crit_embed_mix(const float* proj_tm, const int64_t* ids, const float* W, const float* bias, const float* eps, float* h,
                        int ng, int B, int L, int V, void* stream);
int dlsg_crit_embed_mix_bwd(const float* ch, const float* eps, float* dhr, float* dhf_tm, int ng, int B, int L, void* stream);
int dlsg_crit_vocab_scatter(const float* dhr, const int64_t* ids, float* dW, int rows, int V, void* stream);

/* ResBlock head (sublayer.py:110-119; its ReLU is in place, so the skip carries relu(x)): z = x * [ref > 0];
 * y = z (+ bias_scale * bias); taps[i, l, 3 c + k] = z[i, l + k - 1, c] (zero outside the caption): the three shifted copies that
 * turn Conv1d(512, 512, 3, padding = 1) into ONE product with conv.weight viewed as (512, 1536).  x, ref, y (n, L, 512), taps (n, L, 1536).
 * bwd: dx = (dy + sum_k dtaps[i, l - k + 1, 3 c + k]) * [ref > 0]. */
int dlsg_crit_relu_taps(const float* x, const float* ref, const float* bias, float bias_scale, float* y, float* taps, int n, int L,
                        void* stream);
int dlsg_crit_relu_taps_bwd(const float* dy, const float* dtaps, const float* ref, float* dx, int n, int L, void* stream);

/* (tanh +) LayerNorm with dropouts: z = drop_pre(x); t = pre_tanh ? tanh(z) : z; y = drop_post(LN(t) gamma + beta), rows of N = 64..1024
 * columns (N % 64 == 0), `groups` <= 4 same-shape blocks of `rows` rows with their own arrays (the critic's two proposal heads side
 * by side); block g uses dropout sites site_* + g; the mask of element (r, j) is keyed by (row0 + r) * N + j.
 *   bwd : dy = sum of ndy <= 3 arrays; dx (rows [acc_lo, acc_hi) of every block added to), dgamma / dbeta (NULL: not wanted;
 *         extra[g] (2, N), optional, is added to (dgamma, dbeta)); ws = dlsg_cln_ws_floats(rows, N) * groups floats of scratch
 *   bwd2: U = tangent of x -> gdy = tangent of y, gx = derivative of dx, gpart[g] (2, N) = derivative of (dgamma, dbeta) */
#define DLSG_CLN_MAXG 4
typedef struct {
    const float* x[DLSG_CLN_MAXG]; const float* gamma[DLSG_CLN_MAXG]; const float* beta[DLSG_CLN_MAXG];
    float* y[DLSG_CLN_MAXG];
    const float* dy[3][DLSG_CLN_MAXG]; float* dx[DLSG_CLN_MAXG];
    float* dgamma[DLSG_CLN_MAXG]; float* dbeta[DLSG_CLN_MAXG]; const float* extra[DLSG_CLN_MAXG];
    const float* U[DLSG_CLN_MAXG]; float* gx[DLSG_CLN_MAXG]; float* gdy[DLSG_CLN_MAXG]; float* gpart[DLSG_CLN_MAXG];
    float* ws;
    int32_t rows, N, groups, pre_tanh, ndy, acc_lo, acc_hi;
    int32_t defer; /* != 0: dlsg_cln_bwd / dlsg_cln_bwd2 leave the per-workgroup partial sums in ws -- [group][dgamma | dbeta]
                    * [dlsg_cln_ws_floats(rows, N) / (2 N) rows][N], bwd2 fills the dgamma half only (its dbeta is zero) -- and do
                    * not fold them: the caller sums the rows with the other column sums of its step (dlsg_crit_colsum) */
    float eps, p_pre, p_post; uint32_t site_pre, site_post, pad2_;
    uint64_t seed; const uint64_t* seed_ptr; int64_t row0;
} dlsg_cln_args;
int64_t dlsg_cln_ws_floats(int rows, int N);
int dlsg_cln_fwd(const dlsg_cln_args* a, void* stream);
int dlsg_cln_bwd(const dlsg_cln_args* a, void* stream);
int dlsg_cln_bwd2(const dlsg_cln_args* a, void* stream);

/* Masked self-attention core of one caption on rows [K | Q | V] (n, L, 1536) (sublayer.py:66-78 with att_mask[b,i,j] =
 * smask[b,i] smask[b,j], run_gun.py:164-166; smask (B, L), caption i uses smask[i % B]):
 *   w = softmax_j(scale K_i . Q_j, masked entries -9e15), ctx = w V.     bwd: dctx -> dKQV.
 *   bwd2: U (n, L, 1536) tangent of [K | Q | V], dctx fixed, w as the forward saved it -> Uctx (tangent of ctx), gKQV (derivative of
 *         dKQV; w varies with K, Q). */
typedef struct {
    const float* KQV; const float* smask; float* w; float* ctx;
    const float* dctx; float* dKQV;
    const float* U; float* Uctx; float* gKQV;
    int32_t n, B, L, acc_lo, acc_hi, pad_;
    float scale, pad2_;
} dlsg_crit_sa_args;
int dlsg_crit_sa_fwd(const dlsg_crit_sa_args* a, void* stream);
int dlsg_crit_sa_bwd(const dlsg_crit_sa_args* a, void* stream);
int dlsg_crit_sa_bwd2(const dlsg_crit_sa_args* a, void* stream);

/* PSLScore2's word -> proposal graph (layer.py:697-707), both heads per launch: a[h] (n, L, 512) words, e[h] (B, T, 512) proposals
 * of the clips (caption i scores clip i % B):
 *   P = softmax over the words of scale a e^T (n, L, T); adj = P * smask (mask AFTER the softmax, :703-704); wgt = sum_l adj (n, T);
 *   aggpre = adj^T a (n, T, 512).
 *   bwd : d_agg (n, T, 512), d_wgt (n, T) -> da (n, L, 512), de (n, T, 512) per caption (NULL: not wanted; the caller sums a clip's captions)
 *   bwd2: Ua = tangent of a, P as the forward saved it -> Uagg, Uwgt (tangents), ga, ge (derivatives of da, de) */
typedef struct {
    const float* a[2]; const float* e[2]; const float* smask;
    float* P[2]; float* wgt[2]; float* aggpre[2];
    const float* d_agg[2]; const float* d_wgt[2]; float* da[2]; float* de[2];
    const float* Ua[2]; float* Uagg[2]; float* Uwgt[2]; float* ga[2]; float* ge[2];
    int32_t n, B, L, T, acc_lo, acc_hi;
    float scale, pad_;
} dlsg_crit_pattn_args;
int dlsg_crit_pattn_fwd(const dlsg_crit_pattn_args* a, void* stream);
int dlsg_crit_pattn_bwd(const dlsg_crit_pattn_args* a, void* stream);
int dlsg_crit_pattn_bwd2(const dlsg_crit_pattn_args* a, void* stream);

/* Text summary (LatentPSL(512, 1), sublayer.py:189-198, no mask) and the fusion weights (models/model.py:163-165):
 *   adj = softmax_l(words theta) (n, L); u = adj^T words (n, 512); sent = drop(LN(tanh(u))); fus = softmax(sent fusion^T) (n, 2)
 *   bwd : d_fus (n, 2) -> dwords (n, L, 512), part (n, 5, 512) per-caption partials of [dtheta, dgamma, dbeta, dfusion_0, dfusion_1]
 *         (NULL: not wanted)
 *   bwd2: U (n, L, 512) tangent of words -> Ufus, gwords, gpart (n, 5, 512) */
typedef struct {
    const float* words; const float* theta; const float* gamma; const float* beta; const float* fusion;
    float* adj; float* u; float* sent; float* fus;
    const float* d_fus; float* dwords; float* part;
    const float* U; float* Ufus; float* gwords; float* gpart;
    int32_t n, L, acc_lo, acc_hi;
    float eps, p; uint32_t site, pad_;
    uint64_t seed; const uint64_t* seed_ptr; int64_t row0;
} dlsg_crit_tsum_args;
int dlsg_crit_tsum_fwd(const dlsg_crit_tsum_args* a, void* stream);
int dlsg_crit_tsum_bwd(const dlsg_crit_tsum_args* a, void* stream);
int dlsg_crit_tsum_bwd2(const dlsg_crit_tsum_args* a, void* stream);

/* Pair scores, batch means, critic output (sublayer.py:304-306, layer.py:709-714, models/model.py:165-166), heads h = 0, 1:
 *   pair[h][i,t] = sum_c v[h][i % B,t,c] s[h][i,t,c] wc[h][c] + bc[h];  score[h][i] = sum_t pair wgt / sum_t wgt;
 *   both[g][h] = mean over the B captions of set g of score[h] (PSLScore2 ends with a mean over ITS batch);  out[i] = sum_h both[g(i)][h] fus[i][h]
 *   v = tanh(v_pre) (B, T, 512), s = tanh(s_pre) (n, T, 512): the backward returns the gradients of the PRE-activations.
 *   bwd : d_out (n) -> d_fus (n, 2), c_spre[h] (n, T, 512), c_vpre[h] (n, T, 512) per caption (NULL: not wanted), d_wgt[h] (n, T),
 *         part_wc[h] (n, 512) per-caption partials of classify.weight's gradient and dbc (2) (NULL: not wanted); scratch (4 ng + 8) floats
 *   bwd2: ONE caption set (n == B); tangents Uspre[h] (n, T, 512) of s_pre, Uwgt[h] (n, T), Ufus (n, 2) -> the derivatives of bwd's
 *         outputs: g_fus, g_spre, g_vpre, g_wgt, gpart_wc, g_dbc; scratch (2 n + 16) floats */
typedef struct {
    const float* v[2]; const float* s[2]; const float* wc[2]; const float* bc[2]; const float* wgt[2]; const float* fus;
    float* pair[2]; float* score[2]; float* both; float* out;
    const float* d_out; float* d_fus; float* c_spre[2]; float* c_vpre[2]; float* d_wgt[2]; float* part_wc[2]; float* dbc;
    const float* Uspre[2]; const float* Uwgt[2]; const float* Ufus;
    float* scratch;
    int32_t n, B, T, ng, acc_lo, acc_hi;
} dlsg_crit_score_args;
int dlsg_crit_score_fwd(const dlsg_crit_score_args* a, void* stream);
int dlsg_crit_score_bwd(const dlsg_crit_score_args* a, void* stream);
int dlsg_crit_score_bwd2(const dlsg_crit_score_args* a, void* stream);

/* Gradient penalty and the update's loss values (run_gun.py:362-375) from g = d(sum mixed scores)/d(mixed projection) (B, L, 512) and
 * gG = g (W W^T): q_b = sum g gG = |d mixed score_b / d mixed caption_b|^2, gn = sqrt(max(q, 1e-24)), penalty = mean (gn - 1)^2,
 * c_b = d penalty / d q_b (0 where q was clamped).  out (3B): scores of [real | fake | mixed].
 * stats[0..5) = loss_D = mean fake - mean real + 10 penalty, mean real, mean fake, penalty, mean real - mean fake;
 * vseed = 20 c_b gG (= 10 d penalty / d g), gsc = 10 c_b g.  q: B floats of scratch. */
int dlsg_crit_gp(const float* g, const float* gG, const float* out, float* stats, float* vseed, float* gsc, float* q, int B, int L,
                 void* stream);

/* Top-k proposals of a clip by attention mass (layer.py:694-696): head 0 = the first P columns of alpha (B, L, 2P) (row stride lda,
 * clip stride sa), head 1 = the last P; idx (2, B, T) int64 = rows (h B + b) P + p of the (2 B P, .) proposal embeddings, by
 * decreasing sum_l alpha smask (ties: the lower p).  unselect: dst (R, n) row idx[r] = src[r], every other row zero. */
int dlsg_crit_topk(const float* alpha, int64_t sa, int64_t lda, int na, const float* smask, int64_t* idx, int B, int L, int P, int T,
                   void* stream);
int dlsg_crit_unselect(const float* src, const int64_t* idx, float* dst, int rows_src, int rows_dst, int per, int n, void* stream);

/* `count` <= DLSG_CRIT_REDUCE_MAX sums of slabs in one launch: out[i] = scale * sum_{k < nslab} src[k * stride + i], i < n (n, stride
 * multiples of 4, 16-byte aligned): the K-split partial weight gradients of a critic update, folded in slab order. */
#define DLSG_CRIT_REDUCE_MAX 16
typedef struct {
    const float* src; int64_t stride; int64_t n; int32_t nslab; float scale;
    float* out;
} dlsg_crit_reduce_desc;
int dlsg_crit_reduce(const dlsg_crit_reduce_desc* d, int count, void* stream);

/* `count` <= DLSG_CRIT_COLSUM_MAX column sums in one launch: out[j] = scale * (sum_r part[r, j] + sum_r part_b[r, j]) (part_b optional), also written
 * to out_b when set (bias_ih / bias_hh of an LSTM receive the same gradient).  Fixed order of additions.  n <= 2048. */
#define DLSG_CRIT_COLSUM_MAX 48
typedef struct {
    const float* part; int64_t ld; int32_t rows, n;
    const float* part_b; int64_t ld_b; int32_t rows_b, pad_;
    float* out; float* out_b;
    float scale, pad2_;
} dlsg_crit_colsum_desc;
int dlsg_crit_colsum(const dlsg_crit_colsum_desc* d, int count, void* stream);

/* ---------------------------------------------------------------- loss + optimizer (run_gun.py:189-198, :91)
 * Ragged CrossEntropy: row (b,t) counts iff t < lens[b]; loss = mean over counted rows; dlogits written for all
 * rows (zeros for padded ones).  row_loss (B*L) is scratch; loss[0] receives the mean.  time_major: logits and
 * dlogits are laid out (L,B,V) (the decoder's internal layout) instead of (B,L,V); targets stay (B,L). */
int dlsg_ce_ragged(const float* logits, const int64_t* targets, const int64_t* lens, float* dlogits, float* row_loss,
                   float* loss, int B, int L, int V, int time_major, void* stream);
/* dlsg_ce_ragged with one weight per caption (the policy gradient of self-critical training, weights = reward - baseline):
 * dlogits = weights[b] * (softmax - onehot) / ntot, row_loss = weights[b] * CE / ntot, ntot = sum of lens as above.
 * With every weight 1 the results are bit-identical to dlsg_ce_ragged. */
int dlsg_ce_ragged_weighted(const float* logits, const int64_t* targets, const int64_t* lens, const float* weights, float* dlogits,
                            float* row_loss, float* loss, int B, int L, int V, int time_major, void* stream);
/* dlsg_ce_ragged_weighted against a SOFT target row: label smoothing and word-level distillation of an ensemble (Kim & Rush 2016).
 * Rows, layout, the ragged rule and ntot are dlsg_ce_ragged's; weights is optional (NULL: every caption weighs 1).  Per counted
 * row, with p = softmax(x), lse its log-sum-exp and l_m = x_m - lse_m the log-probabilities of teacher m, whose row for student
 * row r is teacher[m] + r * teacher_ld[m] (same row order as logits):
 *   h_j = (1 - smoothing) [j == tgt] + smoothing / V                  (torch's cross_entropy(label_smoothing=))
 *   q_j = sum_m w[m] softmax(x_m)_j                                   mode 0 ("prob"): the weighted mean probability
 *   q_j = exp(a_j) / sum_i exp(a_i),  a_j = sum_m w[m] l_mj           mode 1 ("logprob"): the weighted geometric mean, RENORMALISED
 *                                                                     (around the row maximum of a: finite when members disagree)
 *   r_j = (1 - alpha) h_j + alpha q_j                                 the target row, sums to 1
 *   dlogits_j = (p_j - r_j) weights[b] / ntot
 * loss[0..2] = the sums over the rows, in a fixed order, of weights[b] / ntot times
 *   {sum_j r_j (lse - x_j),  lse - x_tgt,  sum_j q_j (lse - x_j)}: the mixed loss, the plain NLL of the targets (what
 * dlsg_ce_ragged_weighted reports on these logits) and the CrossEntropy against the teacher (0 when M == 0).  row_loss is scratch
 * of 3 * B * L floats.  Padded rows get zero dlogits and zero losses; a target outside [0, V) makes its row's losses and gradient
 * NaN.  teacher, teacher_ld, w (normalised to sum 1), logw = log(w): HOST arrays of M entries, read during the call and passed to
 * the kernel by value (a captured launch keeps them), as dlsg_beam_select_ens takes them; the loss reads w only.  No atomics,
 * fixed-order reductions.  The student row is read three times; a teacher row three times in mode 0, four in mode 1.
 * EINVAL for M outside 0..DLSG_ENS_MAX, mode outside {0, 1}, smoothing outside [0, 1), alpha outside [0, 1], alpha > 0 with M == 0,
 * M > 0 with alpha == 0.  B * L == 0 launches nothing. */
int dlsg_ce_ragged_soft(const float* logits, const int64_t* targets, const int64_t* lens, const float* weights, float* dlogits,
                        float* row_loss, float* loss, int B, int L, int V, int time_major, float smoothing, float alpha,
                        const float* const* teacher, const int64_t* teacher_ld, const float* w, const float* logw, int M, int mode,
                        void* stream);
/* CIDEr-D corpus tables of a training run (self-critical reward on the device; built once by scoring.DeviceCiderD).  An n-gram
 * of word ids w_0..w_{k-1} (k <= 4) is the key sum_j s_j << 16 j with s_j = w_j for j < k and 0xFFFF past the order; only
 * n-grams made of in-vocabulary words are listed.  Corpus table: the sorted keys and their idf, log_n - log(max(1, df)).
 * References: clip c owns references [clip_off[c], clip_off[c + 1]); reference q owns entries [ref_off[q], ref_off[q + 1])
 * (keys sorted, tf-idf weights), its n norms ref_norm[4 q + k] and its length ref_len[q] (bigram count) over ALL of its n-grams,
 * out-of-vocabulary ones included. */
typedef struct {
    const uint64_t* gram_keys; const double* gram_idf;
    const int64_t* clip_off; const int64_t* ref_off; const double* ref_norm; const int32_t* ref_len;
    const uint64_t* ent_keys; const double* ent_w;
    int64_t n_grams;
    double log_n, sigma;
    int32_t n_clips, vocab, n, pad_;
} dlsg_cider_tables;
/* scores[r] = CIDEr-D (x10, Gaussian length penalty sigma, orders 1..n) of row r of ids (int64, row stride ld) against the
 * references of clip clip_idx[r], in float64, as scoring.CiderD scores decode_tokens(ids[r]): the row's words are those before
 * its first end_id (all L without one).  An id outside [0, vocab) is a word outside the vocabulary (it matches no reference
 * n-gram); a clip index outside [0, n_clips), or a clip without references, scores NaN.  One workgroup per row, fixed-order
 * reductions (bit-identical on every launch).  L <= 64. */
int dlsg_cider_d(const int64_t* ids, int64_t ld, int rows, int L, const int32_t* clip_idx, int64_t end_id,
                 const dlsg_cider_tables* t, double* scores, void* stream);
/* self-critical advantages of B clips x n samples: baseline b_i = greedy[i / n] when greedy is set, else the leave-one-out mean
 * (sum_j r[(i / n) n + j] - r_i) / (n - 1); adv[i] = (float)(r_i - b_i); stats = {mean r, mean b, mean lens} (float64).
 * One workgroup, fixed-order sums.  Without greedy n >= 2. */
int dlsg_scst_advantage(const double* rewards, const int64_t* lens, const double* greedy, int B, int n, float* adv, double* stats,
                        void* stream);
/* Consensus (minimum Bayes risk) ranking of the n candidate captions of each of B clips by CIDEr-D against EACH OTHER: no
 * reference table is read, only the corpus idf (gram_keys, gram_idf, log_n), sigma and n of `t`.  Candidate i of clip b is the row
 * ids + (b n + i) ld, its words as in dlsg_cider_d (those before the first end_id, all L without one).
 *   U[b][i][j]     what scoring.CiderD._score gives hypothesis i when candidate j is its clip's only reference: tf-idf vectors on
 *                  the corpus idf (log_n for an n-gram outside the table), sum over n-grams of min(w_i, w_j) w_j divided by both
 *                  norms when both are nonzero, the sigma length penalty on bigram counts, x10 / t->n.  Not symmetric (clipping).
 *   q[b][j]        1 with scores == NULL, else exp((s_j - max over the valid s) / temperature) in double (temperature > 0;
 *                  +infinity weighs every valid candidate 1).  A candidate whose score is -inf or NaN is invalid: weight 0.
 *   expected[b][i] sum_{j != i} q_j U[b][i][j] / sum_{j != i} q_j, added in index order; 0 when that denominator is 0 (n == 1,
 *                  every other candidate invalid); -inf for an invalid candidate.
 *   order[b][:]    the permutation of 0 .. n-1 that sorts expected[b] descending, ties to the lower index.
 * util (B, n, n) float64 receives U and may be NULL; expected (B, n) float64; order (B, n) int64; scores (B, n) float.
 * Ids outside [0, vocab) never index a table; UNLIKE dlsg_cider_d, where such a word matches no reference word, all of them are
 * here one and the same out-of-vocabulary word, which matches itself within a candidate and across candidates, with df = 0
 * (every n-gram that holds it has idf log_n).  One workgroup of 256 per clip, the candidates' vectors staged in n x 4 KiB of
 * dynamic LDS, float64, no atomics, fixed-order sums: bit-identical on every launch.  1 <= n <= 32, 1 <= L <= 64, L <= ld, else
 * DLSG_EINVAL and no launch; B == 0 launches nothing. */
int dlsg_cider_consensus(const int64_t* ids, int64_t ld, int B, int n, int L, int64_t end_id,
                         const dlsg_cider_tables* t, const float* scores, double temperature,
                         double* util, double* expected, int64_t* order, void* stream);
/* Sentence-level BLEU-1..4 and ROUGE_L (beta = 1.2) of row r of ids (rows as in dlsg_cider_d: int64, row stride ld, the words
 * before the first end_id, L <= 64) against the references of clip clip_idx[r], in float64 and in the operation order of
 * scoring.bleu / scoring.rouge_l.  Reference tables (scoring.DeviceCaptionMetrics): clip c owns references [clip_off[c],
 * clip_off[c + 1]), reference q the words ref_words[ref_off[q] .. ref_off[q + 1]) -- vocabulary ids, 0xFFFF for a word outside
 * the vocabulary, which nothing matches; a reference may be longer than 64 words.  An id outside [0, vocab) is a word that
 * matches no reference word but counts in the length.  Outputs, each optional (NULL):
 *   scores (rows, 5)  BLEU-1..4 (clipped against the maximum count over the references, brevity penalty against the closest
 *                     reference length, shorter on ties) and ROUGE_L (best LCS precision and best LCS recall over the references);
 *                     all 0 for an empty row;
 *   stats (rows, 10)  correct[4], guess[4], row length, closest reference length: the integers corpus BLEU sums;
 *   reward (rows)     weights[0] base[r] + weights[1..4] BLEU-1..4 + weights[5] ROUGE_L, added in that order, a term with weight
 *                     exactly 0 left out.  weights: 6 doubles in HOST memory, read during the call; base: float64 per row (the
 *                     rows' CIDEr-D of dlsg_cider_d), may be NULL when weights[0] == 0.
 * A clip index outside [0, n_clips), or a clip without references, gives NaN scores and reward and zero stats.  One workgroup
 * per row, no atomics, fixed-order reductions (bit-identical on every launch).  References pass through LDS DLSG_METRICS_STAGE
 * words at a time; a longer single reference is read from global memory.  vocab in 1..65535; rows == 0 launches nothing. */
#define DLSG_METRICS_STAGE 2048
int dlsg_caption_metrics(const int64_t* ids, int64_t ld, int rows, int L, const int32_t* clip_idx, int64_t end_id,
                         const int64_t* clip_off, const int64_t* ref_off, const uint16_t* ref_words, int n_clips, int vocab,
                         const double* weights, const double* base, double* scores, int32_t* stats, double* reward, void* stream);
/* Corpus figures of rows scored by dlsg_caption_metrics: out[0..3] = corpus BLEU-1..4 from the column sums of stats (64-bit
 * integers; the closing loop of scoring.bleu), out[4] = mean of scores[:, 4] (ROUGE_L), out[5] = mean of base (NaN without base).
 * One workgroup, fixed-order sums.  rows >= 1. */
int dlsg_caption_corpus(const int32_t* stats, const double* scores, const double* base, int rows, double* out, void* stream);
int dlsg_log_softmax(const float* logits, float* out, int rows, int V, void* stream);
/* One beam-search step for every batch item (BeamSearch.search, allennlp_beamsearch.py:140-260, per-node k == k):
 * log-softmax + per-beam top-k over the vocabulary + top-k over the k*k summed candidates, in one launch.
 * logits (B*k, V) rows (ld floats apart); last (B*k) the tokens fed to this step (a beam whose last token is `end`
 * offers only `end` at log-prob 0); last_lp (B*k) running log-probs.  first != 0: step 0 (only beam 0 of each group).
 * Out: pred (B*k) int64 chosen classes, new_lp (B*k), back (B*k) int64 parent beam, rows (B*k) int64 = b*k + back (the
 * gather indices for the recurrent state), ended_count += number of chosen `end` tokens (optional device counter). */
typedef struct {
    const float* logits; int64_t ld;
    const int64_t* last; const float* last_lp;
    int64_t* pred; float* new_lp; int64_t* back; int64_t* rows;
    int32_t* ended_count;
    int32_t B, k, V, end, first, pad_;
} dlsg_beam_select_args;
int dlsg_beam_select(const dlsg_beam_select_args* a, void* stream);
/* dlsg_beam_select at step t (first != 0 exactly when t == 0) with a token history that travels with the beams and two bans.
 * hist_in / hist_out (B*k, L) int64 rows, two buffers that do not overlap, used ping-pong, L <= 64: new beam c gets its parent's row of
 * hist_in with hist[t] = pred and `end` at every position after t (step 0 reads no hist_in and writes whole rows), so after the
 * last step a row is the end-padded caption of its beam.  no_repeat_ngram = g >= 1: a live beam with history h may not choose
 * class c if an i <= t - g exists with h[i .. i+g-2] == h[t-g+1 .. t-1] and h[i+g-1] == c.  min_len: `end` is banned at steps
 * t < min_len.  A banned class has log-prob -inf; the log-sum-exp stays that of the whole row; a beam that has ended offers
 * `end` at log-prob 0 whatever the bans.  g = 0, min_len = 0: pred, new_lp, back, rows, ended_count are the bits of
 * dlsg_beam_select. */
int dlsg_beam_select_hist(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                          int no_repeat_ngram, int min_len, void* stream);
/* dlsg_beam_select_hist for an ensemble of M members that decode one caption: a live beam's V candidate values are combined from M
 * logit rows, logits[m] + r * ld[m] for beam row r (a->logits and a->ld are ignored).  With l_m = x_m - lse_m, lse_m the row's
 * log-sum-exp in the order dlsg_beam_select_hist takes it, per class, in member order and float32:
 *   mode 0 ("prob"):     c = mx + logf(sum_m expf(v_m - mx)), v_m = l_m + logw[m], mx = max_m v_m (-inf when mx is): the log of
 *                        the weighted mean of the members' probabilities;
 *   mode 1 ("logprob"):  c = sum_m w[m] * l_m, from 0: the weighted mean of their log-probabilities, not renormalised.
 * The k best unbanned c of the row (larger first, ties to the lower class) are offered at c + last_lp; the bans, ended beams, the
 * k*k merge, pred / new_lp / back / rows, the history and ended_count are those of dlsg_beam_select_hist.  With M == 1, w = {1},
 * logw = {0} either mode gives c = x - lse, the value dlsg_beam_select_hist ranks by.  logits, ld, w (normalised to sum 1),
 * logw = log(w): HOST arrays of M entries, read during the call and passed to the kernel by value (a captured launch keeps them).
 * EINVAL for M outside 1..DLSG_ENS_MAX, mode outside {0, 1}, k outside 1..8, L > 64.  Each member row is read three times. */
#define DLSG_ENS_MAX 8
int dlsg_beam_select_ens(const dlsg_beam_select_args* a, const float* const* logits, const int64_t* ld, const float* w,
                         const float* logw, int M, int mode, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                         int no_repeat_ngram, int min_len, void* stream);
/* dlsg_beam_select_ens for diverse (group) beam search (Vijayakumar et al. 2016).  The k beams of a clip are `groups` = G groups of
 * k' = k / G: group y owns rows b*k + y*k' .. b*k + y*k' + k' - 1 on input and on output, and a beam's parent is a row of its own
 * group.  Phase 1 is dlsg_beam_select_ens's: every input row's k best (c, class) -- combined over the M members in `mode`, the two
 * bans, ties to the lower class, an ended row offers only `end` at 0 -- each offered at lp = c + last_lp[row] (float32).  At step 0
 * only the clip's first row is read; its list serves every group, with the group's first row as parent.  Phase 2, the groups in
 * order y = 0 .. G-1, with a count cnt[class] that starts empty at every step: the candidates of y are the k' * k entries of its rows'
 * lists (row within the group, then rank); key = lp if the parent row has ended or cnt[class] == 0, else lp - diversity * cnt[class]
 * in float32 (the product rounded, then the difference), and -inf for diversity = +inf.  The k' best keys are chosen, larger first,
 * ties to the lower candidate; a -inf key is no candidate, and a slot q left over takes candidate q of the group with new_lp = -inf.
 * Output slot o = b*k + y*k' + q: pred = the class, new_lp = lp -- NOT the key: the penalty steers the choice only, so the log-probs
 * stay comparable across groups and with the other searches --, back = the parent's index within the clip, rows = b*k + back,
 * hist_out[o] and ended_count as dlsg_beam_select_hist.  After y has chosen, each of its picks (not a left-over slot) whose parent
 * was live adds one to cnt[its class] (at step 0 every pick): an `end` that continues an ended beam is neither penalised nor
 * counted, a fresh `end` counts like any word.  Penalties only lower values and at most k - k' classes are counted, so the k' best
 * keys of a group lie inside its rows' k best: the vocabulary is read exactly as by dlsg_beam_select_ens.  groups == 1 gives that
 * call's bits.  One workgroup per clip, phase 2 in one wave; no atomics but ended_count's; deterministic.
 * EINVAL for what dlsg_beam_select_ens refuses, groups < 1, k % groups != 0, diversity negative or NaN. */
int dlsg_beam_select_groups(const dlsg_beam_select_args* a, const float* const* logits, const int64_t* ld, const float* w,
                            const float* logw, int M, int mode, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                            int no_repeat_ngram, int min_len, int groups, float diversity, void* stream);
/* dlsg_beam_select_hist for stochastic beam search (Kool, van Hoof & Welling 2019): the step that makes the k beams of a clip an
 * ordered sample WITHOUT replacement from the model.  a, hist_in / hist_out, L, t, no_repeat_ngram, min_len as dlsg_beam_select_hist
 * takes them, but last_lp / new_lp carry phi, the float32 log-prob of the prefix under the tempered model renormalised over the
 * unbanned classes, and G_in / G_out (B*k) float64, two buffers used ping-pong like them, carry the prefix's perturbed value.  A
 * live row r with phi = last_lp[r], T = G_in[r] (step 0: only the clip's first row is read, phi = 0 and T = the root's own Gumbel(0)
 * noise, in float64 from the hash keyed (seed, site_sample, r * V) -- a root pinned to 0 would draw the same captions but condition
 * the largest perturbed value on being 0, and the threshold would no longer give unbiased importance weights): z_j = logits[r, j] *
 * (1 / temperature) in float32; a banned class, a NaN and a -inf logit count as -inf; lse = the log-sum-exp of z over the others, in
 * one pass with an online (max m, sum s); key_j = z_j - log(-log u_j), the float32 key of dlsg_sample_embed, u_j from the counter
 * hash keyed (seed, site_sample, ((t+1) * B*k + r) * V + j) -- with k == 1 the key that call ranks by at row0 = (t+1) * B, so the
 * one-beam search draws its word.  The row's k largest keys (ties to the lower class) are its children; for those only, in float64
 * with the noise of the same 24 hash bits: g_j = phi + (z_j - lse) + noise_j, Z = their maximum, and
 *   v = T - g_j + log1mexp(g_j - Z),  G_j = T - max(0, v) - log1p(exp(-|v|)),  log1mexp(a) = a > -ln 2 ? log(-expm1(a)) : log1p(-exp(a))
 * -- the children's perturbed values given that their maximum is T; the largest child gets T exactly.  A child's phi is last_lp +
 * ((z_j - m) - log s) in float32, the log-prob dlsg_sample_embed reports.  A row that has ended offers `end` with its phi and its T
 * unchanged.  The clip's k new beams are the k largest G_j among the k*k candidates (row, then rank), larger first, ties to the
 * lower candidate, so the output rows of a clip are in sampling order; with fewer than k finite candidates a slot takes phi = -inf
 * and G = -inf.  Out: pred, new_lp, G_out, back, rows, hist_out, ended_count.  seed_ptr (optional, device) is added to seed at run
 * time: a replayed graph draws afresh.  One workgroup per clip, one wave per row; no atomics but ended_count's; deterministic.
 * EINVAL for what dlsg_beam_select_hist refuses, temperature <= 0 or NaN, G_out NULL, t > 0 with G_in NULL or G_in == G_out. */
int dlsg_beam_select_gumbel(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                            int no_repeat_ngram, int min_len, float temperature, uint64_t seed, const uint64_t* seed_ptr,
                            uint32_t site_sample, const double* G_in, double* G_out, void* stream);
/* dlsg_beam_select_hist for lexically constrained beam search (dynamic beam allocation, Post & Vilar 2018; Anderson et al. 2017): a
 * caption must contain a word of every constraint of its clip.  cons (B, C, W) int64, device: cons[b, c] is one constraint of clip b,
 * a set of alternative class ids (disjunctive); an entry outside [0, V) is padding and matches nothing, a constraint without a
 * valid entry is absent; clips may differ in their number C_b of present constraints.  A beam with history h[0..t-1] has MET
 * constraint c iff some h[i], i < t, is a valid entry of cons[b, c]: the mask `met` (bit c) is recomputed from the row of hist_in
 * at every step -- no state beside the history --, one word may meet several constraints, step 0 starts empty, unmet = present & ~met.
 * a, hist_in / hist_out, L, t, no_repeat_ngram, min_len, the log-softmax, the (value, index) order and step 0 reading only the
 * clip's first row are dlsg_beam_select_hist's.  A live row's ban list is that call's, and `end` too while unmet != 0: a beam ends
 * only with every constraint met.  A live row offers two lists.  A: its k best unbanned classes at (x - lse) + last_lp, as
 * dlsg_beam_select_hist offers them.  B: one slot per constraint c < C; for an unmet c the best valid entry of cons[b, c] that is
 * not banned and whose logit is > -inf (a NaN fails), larger logit first, ties to the lower class id, at the same float32
 * (x - lse) + last_lp with the whole row's lse; the slot is empty (-inf, no candidate) if c is met or absent, if no word qualifies,
 * or if the class already is in the row's list A or in an earlier slot c' < c of the row (the clip would get one beam twice).  An
 * ended row offers `end` at its own log-prob in A and nothing in B.  Every candidate above -inf (a NaN is none) has a bank:
 * popcount(parent's met | {c: its class is a valid entry of cons[b, c]}), by one rule for both lists.  Allocation: candidate index =
 * list A (row, then rank), then list B (row, then constraint); repeat until k output slots are filled or no candidate is left: for
 * bank = C down to 0 the best candidate left in the bank (larger value, ties to the lower candidate index) takes the next output
 * slot, an empty bank is skipped.  A slot q left over takes candidate q of list A with new_lp = -inf.  Out, in pick order: pred,
 * new_lp (the candidate's log-prob, nothing added for the bank), back, rows, hist_out, ended_count as dlsg_beam_select_hist;
 * met_out (B*k) int32, optional: the new beam's mask with the chosen word, 0 for a left-over slot.  While a beam of the clip has an
 * unmet constraint with a finite-logit word, the highest bank among the clip's beams rises by one per step, and the top bank is
 * served first, so from step C_b on a beam with every constraint met exists and stays.  With C == 0, cons NULL or every constraint
 * of a clip absent there is one bank and the clip's outputs are the bits of dlsg_beam_select_hist.  Not covered: ordered
 * constraints, the same word twice; multi-word phrases are dlsg_beam_select_phrases'.  One workgroup per clip, one wave per row, the allocation in one wave; no
 * atomics but ended_count's; deterministic.  EINVAL for what dlsg_beam_select_hist refuses, C < 0, C > DLSG_CONS_MAX, and with
 * C > 0: W < 1, W > DLSG_CONS_ALT, cons NULL. */
#define DLSG_CONS_MAX 8   /* constraints per clip */
#define DLSG_CONS_ALT 8   /* alternative words per constraint */
int dlsg_beam_select_cons(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                          int no_repeat_ngram, int min_len, const int64_t* cons, int C, int W, int32_t* met_out, void* stream);
/* dlsg_beam_select_cons whose constraints are sets of alternative PHRASES: a caption must contain, as contiguous words, a phrase of
 * every constraint of its clip.  phr (B, C, W, P) int64, device: C <= DLSG_CONS_MAX constraints per clip, W <= DLSG_CONS_ALT
 * alternatives per constraint, 1 <= P <= DLSG_PHRASE_MAX words per alternative.  Alternative a is the leading run of entries in
 * [0, V): its length n(a) is the number of such entries before the first entry outside that range, whatever follows is ignored,
 * n(a) = 0 means absent; a constraint is present iff it has a valid alternative; clips may differ in all of this.
 * The state of a row is recomputed from its history h[0..t) at every step, nothing is carried:
 *   a OCCURS if h[i..i+n) == a for some i; constraint c is MET if a valid alternative of c occurs (`met`: the bit mask);
 *   unmet = present & ~met;
 *   the PROGRESS p(a) of a is the largest j <= min(n(a) - 1, t) such that the last j tokens of h equal a[0..j) -- the longest
 *   border: for "x x y" behind "... x x x" it is 2, not 0;
 *   the progress q of a row is the maximum of p(a) over the valid alternatives of its unmet constraints, 0 without any;
 *   the BANK of a row is the pair (popcount(met), q), ordered lexicographically.
 * The step is dlsg_beam_select_hist's (log-softmax, (value, index) order, bans, step 0 reading the clip's first row) with the three
 * additions of dlsg_beam_select_cons, generalised.  (1) `end` is banned for a live row while unmet != 0.  (2) List B: a live row
 * offers, beside list A, one slot per unmet constraint.  Every valid alternative a of the constraint proposes the word
 * u = a[p(a)], with the gain s(a) = P if p(a) + 1 == n(a) (the word completes the phrase), else p(a) + 1; a proposal is out if u is
 * banned or its logit is -inf or NaN; the slot takes the proposal with the largest gain, then the larger logit, then the lower
 * class, at (x - lse) + last_lp in the float32 operations of list A; it is empty if that class already is in the row's list A or
 * in an earlier slot of the row (no fall-through to the next proposal).  (3) Merge: every candidate (parent row, class u) above
 * -inf, of either list, has the bank of the history h_parent + [u] by the definitions above; a candidate `end` changes neither
 * met nor progress.  The k output slots are filled round-robin over the non-empty banks from the highest bank down, each time with
 * the best candidate left in the bank: larger value first, ties to the lower candidate index (list A before list B, list B indexed
 * by row, then constraint); left-over slots as dlsg_beam_select_cons fills them.  new_lp is the plain log-prob.  met_out (B*k)
 * int32, optional: the new beam's mask; bank_out (B*k) int32, optional: popcount(met) * DLSG_PHRASE_MAX + q; both 0 for a
 * left-over slot.
 * One word may serve several constraints ("hot dog house" meets "hot dog" and "dog house").  Widening C, W or P with entries of -1
 * changes no output bit.  With P == 1 the launch returns the bits of dlsg_beam_select_cons; with C == 0, phr NULL or only absent
 * constraints those of dlsg_beam_select_hist.  A row of the clip's highest bank whose deciding constraint has a proposal that is
 * not out offers a candidate of a strictly higher bank, and the highest bank is served first: with no_repeat_ngram == 0 and finite
 * logits some beam meets every present constraint within C_b * n_max_b words (n_max_b: the clip's longest phrase) and is never
 * dropped.  Progress can be thrown away -- completing a one-word constraint mid-phrase outranks continuing the phrase --, hence not
 * the sum of the lengths.  With an n-gram ban the next word of a phrase can be banned without the phrase having occurred
 * (g = 2, "a b c" behind "b c ... a b"): best effort, a beam that cannot finish runs on without `end`.  Not covered: ordered
 * constraints, the same phrase twice, phrases of more than DLSG_PHRASE_MAX words.  One workgroup per clip, one wave per row, the
 * merge in one wave; no atomics but ended_count's, a fixed reduction order: two launches give equal bits.  EINVAL for what
 * dlsg_beam_select_cons refuses, and with C > 0 for P < 1 or P > DLSG_PHRASE_MAX. */
#define DLSG_PHRASE_MAX 4   /* words per phrase */
int dlsg_beam_select_phrases(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                             int no_repeat_ngram, int min_len, const int64_t* phr, int C, int W, int P, int32_t* met_out,
                             int32_t* bank_out, void* stream);
/* dlsg_beam_select_ens with EXCLUSIONS: words and phrases a caption must not contain.  excl_shared (NS, P) int64, device: NS <=
 * DLSG_EXCL_SHARED entries that hold for every clip; excl_clip (B, NC, P) int64, device: NC <= DLSG_EXCL_CLIP entries of each
 * clip's own; 1 <= P <= DLSG_PHRASE_MAX; either table may be NULL with its count 0.  An entry e is the leading run of ids in
 * [0, V) of its row of P words -- it is cut at the first id outside that range, as dlsg_beam_select_phrases cuts an alternative --,
 * n its length, n == 0: absent.  For a live row at step t with history h[0 .. t), the word e[n-1] is banned iff n - 1 <= t and
 * h[t-n+1 .. t-1] == e[0 .. n-2]: a one-word entry bans its word at every step (`<unk>`), the two-word entry (w, end) forbids a
 * caption to stop behind w (a bad ending).  The context never matches the start token, which is not part of the history, and an
 * entry longer than the caption so far bans nothing.  These bans join the row's list behind those of no_repeat_ngram and min_len
 * (a word may stand there twice); a banned class counts as -inf in the row's k best while the log-sum-exp stays that of the whole
 * row; a row that has ended is untouched.  Everything else -- the members and their combination in `mode`, the (value, index)
 * order, step 0 reading the clip's first row, the k*k merge, pred / new_lp / back / rows, hist_out, ended_count -- is
 * dlsg_beam_select_ens's: with NS == NC == 0 the launch returns that call's bits, and with M == 1, w = {1} besides those of
 * dlsg_beam_select_hist.  One workgroup per clip, one wave per row; no atomics but ended_count's; deterministic.  EINVAL for what
 * dlsg_beam_select_ens refuses, NS outside 0..DLSG_EXCL_SHARED, NC outside 0..DLSG_EXCL_CLIP, a count above 0 with a NULL table,
 * and, with a count above 0, P outside 1..DLSG_PHRASE_MAX. */
#define DLSG_EXCL_SHARED 64   /* excluded entries shared by all clips */
#define DLSG_EXCL_CLIP 32     /* excluded entries of one clip */
int dlsg_beam_select_excl(const dlsg_beam_select_args* a, const float* const* logits, const int64_t* ld, const float* w,
                          const float* logw, int M, int mode, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                          int no_repeat_ngram, int min_len, const int64_t* excl_shared, int NS, const int64_t* excl_clip, int NC,
                          int P, void* stream);
/* dlsg_sample_filter_embed under EXCLUSIONS: that call's arguments, then the two tables of dlsg_beam_select_excl -- excl_shared
 * (NS, P) for every row, excl_clip (rows / rows_per_clip, NC, P), of which row r reads the entries of clip r / rows_per_clip (the n
 * samples of a clip are consecutive rows).  With h the row's own words (h[i] = hist[i * hist_stride + r], i < t) the word e[n-1] of
 * an entry e of length n is banned by dlsg_beam_select_excl's rule: n - 1 <= t and h[t-n+1 .. t-1] == e[0 .. n-2].  These bans join
 * those of step 1 of dlsg_sample_filter_embed (a word may stand in the list twice) and, like them, come before top_k and top_p and
 * RENORMALISE: logp is the log-probability over the words that are left, kept their number behind top_k / top_p.  (The beam step
 * does not renormalise.)  A word's noise does not depend on the bans: the launch draws what dlsg_sample_filter_embed draws from
 * the same rows with the logits of the words the tables ban set to -inf, with that call's ids, lens, kept and embedded rows.
 * temperature 0: the first maximum over the words that are not banned.  A row with no word left gives word 0 and kept 0.  A row
 * that has drawn end_id goes on drawing under the same rule.  hist may be NULL only when no_repeat_ngram == 0 and NS + NC == 0,
 * or t == 0.  The tables and the longer list take about 3 KB of LDS beside the row's V floats.  No atomics; two launches, or a
 * launch and a graph replay, give the same bits; NS == NC == 0 gives the bits of dlsg_sample_filter_embed.  EINVAL for what
 * dlsg_sample_filter_embed refuses, for what dlsg_beam_select_excl refuses of its tables, rows_per_clip < 1, rows not a multiple
 * of rows_per_clip, and t > 0 with an entry and hist NULL or hist_stride < rows. */
int dlsg_sample_excl_embed(const float* logits, int64_t ld, int V, float temperature, const float* E, int64_t* ids_out, float* out,
                           int64_t ldo, int W, float* logp, int64_t* lens, int t, int64_t end_id, int rows, float p, uint64_t seed,
                           uint32_t site_word, uint32_t site_sample, int64_t row0, const uint64_t* seed_ptr, int top_k, float top_p,
                           int min_len, int no_repeat_ngram, const int64_t* hist, int64_t hist_stride, int32_t* kept,
                           const int64_t* excl_shared, int NS, const int64_t* excl_clip, int NC, int P, int rows_per_clip, void* stream);
/* dlsg_beam_select_gumbel under EXCLUSIONS: that call's arguments, then the two tables as dlsg_beam_select_excl takes them
 * (excl_clip (B, NC, P): the entries of the clip whose k rows the workgroup holds).  A live row's banned classes are those of
 * no_repeat_ngram and min_len and the last words of the entries its history row leads up to, by dlsg_beam_select_excl's rule; as in
 * dlsg_beam_select_gumbel a banned class counts as -inf in the keys AND in the log-sum-exp, so phi stays the log-prob under the
 * model renormalised over the words that are left.  The launch returns what dlsg_beam_select_gumbel returns on the same rows with
 * the logits of those words set to -inf; a row that has ended is untouched; NS == NC == 0 gives that call's bits.  EINVAL for what
 * dlsg_beam_select_gumbel refuses and for what dlsg_beam_select_excl refuses of its tables. */
int dlsg_beam_select_gumbel_excl(const dlsg_beam_select_args* a, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                                 int no_repeat_ngram, int min_len, float temperature, uint64_t seed, const uint64_t* seed_ptr,
                                 uint32_t site_sample, const double* G_in, double* G_out, const int64_t* excl_shared, int NS,
                                 const int64_t* excl_clip, int NC, int P, void* stream);
/* After the last step: the n <= k best beams of every clip by score = lp / len^alpha (computed in double, stored as float),
 * descending, ties to the lower beam.  hist (B*k, L) the final history, lp (B*k) the final log-probs; len = tokens up to and
 * including the first `end`, L without one.  Out: ids (B, n, L) int64, scores (B, n), lens (B, n) int64.  One wave per clip. */
int dlsg_beam_finalize(const int64_t* hist, const float* lp, int B, int k, int L, int64_t end, double alpha, int n,
                       int64_t* ids, float* scores, int64_t* lens, void* stream);
/* The log-probability of GIVEN captions under one model or an ensemble of M members, from teacher-forced logits: what the
 * searches report for captions of their own, for any caption.  Row (t, r) of member m is logits[m] + t * ld_t[m] + r * ld_r[m], V
 * floats (time-major (L, R, V) and (R, L, V) alike); ids holds R rows of L int64, ids_ld apart, word t of row r being what position
 * t should predict.  logits, ld_t, ld_r, w (normalised to sum 1), logw = log(w): HOST arrays of M entries, read during the call and
 * passed to the kernel by value (a captured launch keeps them), as dlsg_beam_select_ens takes them.
 *   len_r          lens_in == NULL: the tokens up to and including the first `end`, L without one (dlsg_beam_finalize's rule);
 *                  else lens_in[r] clamped to [0, L].  lens_out[r] = len_r.
 *   tok_lp[r, t]   t < len_r: the combined log-probability c of class ids[r, t], in the float32 operations and order of
 *                  dlsg_beam_select_ens: per member lse_m (strided maximum, wave maximum, strided exponential sum, wave sum,
 *                  logf(sum) + max), then mode 0 or mode 1 over the members in member order.  With M == 1 it is x - lse, the bits
 *                  dlsg_beam_select_hist adds to last_lp for that class.  t >= len_r: 0.  Only the rows t < len_r are read.
 *   lp[r]          the float32 sum in step order, acc = tok_lp[t] + acc from 0 at t = 0 (how the searches accumulate new_lp);
 *   scores[r]      lp / len_r^alpha, computed in double, stored as float (dlsg_beam_finalize's); len_r == 0: lp = scores = 0.
 *   tok_rank[r, t] t < len_r: the number of classes j with c_j > c_tgt, or c_j == c_tgt and j < tgt (the searches' order: 0 is
 *                  the word a greedy decode chooses here).  With M == 1 the comparison is on the raw logits, as the one-model step
 *                  ranks: exact, whatever the rounding of lse.  A class whose c is NaN is not counted (a NaN target has rank 0).
 *                  t >= len_r: -1.  NULL skips its work: with M == 1 the count rides on the maximum pass, with M > 1 it reads
 *                  every member row a third time.
 * A target outside [0, V) indexes nothing: tok_lp NaN, tok_rank -1, so lp and scores are NaN (dlsg_ce_ragged_soft's rule).  A
 * target whose logit is -inf has tok_lp -inf.  A member row that is all -inf or holds a NaN has lse_m = NaN, as in
 * dlsg_beam_select_ens, so every l_m of the row is NaN: with M == 1 and in mode 1 tok_lp is NaN; in mode 0 the maximum over the
 * members skips a NaN, so tok_lp is NaN where another member gives the class a finite value and -inf where none does.
 * tok_lp, tok_rank ((R, L) dense), lp, scores, lens_out ((R)) are each optional (NULL).  One launch, one workgroup per caption, one
 * wave per position, no atomics, fixed-order reductions: two launches give equal bits.  EINVAL and no launch for M outside
 * 1..DLSG_ENS_MAX, mode outside {0, 1}, L outside 1..64, V < 1, alpha negative or NaN, ids_ld < L.  R == 0 launches nothing. */
int dlsg_seq_logprob(const float* const* logits, const int64_t* ld_t, const int64_t* ld_r, const float* w, const float* logw, int M,
                     int mode, const int64_t* ids, int64_t ids_ld, const int64_t* lens_in, int R, int L, int V, int64_t end,
                     double alpha, float* tok_lp, int32_t* tok_rank, float* lp, float* scores, int64_t* lens_out, void* stream);
/* A FORCED PREFIX behind a history step: launched behind the step's select launch (any of dlsg_beam_select_hist / _ens / _excl /
 * _cons / _phrases) on the same argument block `a`, the same hist_in / hist_out, L and t, with the members as
 * dlsg_beam_select_ens takes them (a single model: M == 1, w = {1}, logw = {0}; a->logits and a->ld are ignored).  prefix (B, P)
 * int64: clip b's prefix is the leading run of ids in [0, V) of its row, p_b words (0 .. P); any other id, normally -1, ends it.
 * One workgroup of one wave per clip.  t >= p_b: the workgroup returns and nothing of the clip is written -- the select launch's
 * outputs stand.  t < p_b, with w = prefix[b, t] and the clip's first row b*k as the parent: all k output slots b*k + c get
 * pred = w, back = 0, rows = b*k and the history row hist_in[b*k][0 .. t), w, then `end` (dlsg_beam_select_hist's rule); slot 0
 * gets new_lp = c(w) + (t == 0 ? 0 : last_lp[b*k]), c(w) the combined value of class w on row b*k exactly as dlsg_seq_logprob
 * computes tok_lp (with M == 1 x - lse, the bits dlsg_beam_select_hist adds for that class); slots 1 .. k-1 get new_lp = -inf, so
 * the first free step expands beam 0 alone, as step 0 does.  No ban applies to a forced word; a forced word whose value is -inf or
 * NaN gives the clip that log-prob.  ended_count is not touched.  EINVAL and no launch for k outside 1..8, L outside 1..64, t
 * outside [0, L), P outside 0..L-1, M outside 1..DLSG_ENS_MAX, mode outside {0, 1}, prefix NULL with P > 0, hist_out NULL, and
 * t > 0 with hist_in NULL or equal to hist_out.  P == 0, B == 0 or t >= P launches nothing. */
int dlsg_beam_force_prefix(const dlsg_beam_select_args* a, const float* const* logits, const int64_t* ld, const float* w,
                           const float* logw, int M, int mode, const int64_t* hist_in, int64_t* hist_out, int L, int t,
                           const int64_t* prefix, int P, void* stream);
/* A FORCED PREFIX behind a sampled step: launched behind dlsg_sample_embed, dlsg_sample_filter_embed or dlsg_sample_excl_embed
 * on that call's logits, E, ids_out, out, logp, lens, t, temperature, p, seed / seed_ptr, site_word and row0.  prefix
 * (rows / rows_per_clip, P) int64 as dlsg_beam_force_prefix reads it; row r reads clip r / rows_per_clip.  A row whose clip has
 * p_b <= t returns at once.  A forced row gets ids_out[r] = w = prefix[., t]; logp[r] = the log-probability of w under
 * softmax(logits[r] / temperature) (temperature 0: the untempered softmax) in the operations of dlsg_sample_embed, so forcing the
 * word that call drew leaves its bits; no control of the filtered steps applies; out[r] = E[w] under the word-dropout stream
 * (seed, site_word, row0 + r); lens[r] = L (a prefix holds no end_id and every earlier step of the row was forced, so it was L
 * on entry to step t); kept[r] = 1 (kept may be NULL).  EINVAL and no launch for V < 1, W < 0, temperature < 0, L < 1, t outside
 * [0, L), P outside 0..L-1, prefix NULL with P > 0, rows_per_clip < 1 and rows not a multiple of it.  rows == 0 or t >= P
 * launches nothing. */
int dlsg_sample_force_prefix(const float* logits, int64_t ld, int V, float temperature, const float* E, int64_t* ids_out, float* out,
                             int64_t ldo, int W, float* logp, int64_t* lens, int t, int rows, float p, uint64_t seed,
                             uint32_t site_word, int64_t row0, const uint64_t* seed_ptr, const int64_t* prefix, int P,
                             int rows_per_clip, int L, int32_t* kept, void* stream);
/* dst_i[r,:] = src_i[rows[r],:] (dense rows of n[i] floats) for count <= 4 arrays in one launch */
typedef struct {
    const float* src[4]; float* dst[4]; int32_t n[4];
    const int64_t* rows; int32_t nrows, count;
} dlsg_gather_multi_args;
int dlsg_gather_rows_multi(const dlsg_gather_multi_args* a, void* stream);
/* torch.optim.Adam semantics (no weight decay, no amsgrad); step = 1-based step count; grad_scale folds 1/world */
int dlsg_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, int step,
              float grad_scale, const float* hyper, const int32_t* guard, void* stream);
/* hyper (optional, device): {lr / (1 - b1^step), sqrt(1 - b2^step)} -- overrides lr/step so a captured graph can be
 * replayed with a new step count.  guard (optional, device): the launch updates nothing when *guard != 0 -- the `err` word of the
 * persistent recurrent kernels (dlsg_bilstm_*, dlsg_lstm_seq): a step whose hand-off timed out has invalid gradients. */

/* ---------------------------------------------------------------- gradient clipping by global norm, on the device
 * torch.nn.utils.clip_grad_norm_ / clip_grad_value_ between the backward and the update, as three launches that can be captured
 * with the step (no host read of the norm): dlsg_grad_sumsq per trainable range of the gradient arena, dlsg_clip_coef once,
 * dlsg_adam_clipped per range.  No atomics anywhere: the same gradient bits give the same record bits on every launch, every
 * graph replay and every rank of a data-parallel job (which reduce the same all-reduced sum), so no collective is needed.
 *
 * dlsg_grad_sumsq: slots[w] = workgroup w's share of sum g[i]^2 over g[0..n), w < DLSG_GRAD_SUMSQ_SLOTS; every element is squared
 *   and accumulated in float64 (the square of a float is exact there), each workgroup reduces in a fixed order, a workgroup
 *   without elements writes 0 -- the caller never zeroes the slots.  The grid does not depend on n.  g may start at any float
 *   (16-byte loads over the aligned body, scalar head and tail); one launch per range, each into its own block of slots.
 * dlsg_clip_coef: one workgroup sums slots[0..count) in a fixed order and writes record[0..DLSG_CLIP_RECORD_FLOATS):
 *   [DLSG_CLIP_NORM]      (float) (grad_scale * sqrt(sum)): the norm of the averaged gradient
 *   [DLSG_CLIP_COEF]      min(1, max_norm / (norm + 1e-6))  (clip_grad_norm_'s formula); max_norm = +inf: 1, nothing is clipped
 *   [DLSG_CLIP_NONFINITE] 1.0 when the norm is inf or NaN, else 0.0; then coef = 0 and *skipped (optional, device) goes up by one.
 * dlsg_adam_clipped: dlsg_adam on gi = (g * grad_scale) * record[DLSG_CLIP_COEF], then clamped to +-clip_value when clip_value > 0.
 *   record (optional, device): with record[DLSG_CLIP_NONFINITE] != 0 the launch updates nothing, exactly as under `guard`.
 *   A record with coef 1.0 (or none) and clip_value 0 gives dlsg_adam's bits. */
#define DLSG_GRAD_SUMSQ_SLOTS 1024
#define DLSG_CLIP_NORM 0
#define DLSG_CLIP_COEF 1
#define DLSG_CLIP_NONFINITE 2
#define DLSG_CLIP_RECORD_FLOATS 4
int dlsg_grad_sumsq(const float* g, int64_t n, double* slots, void* stream);
int dlsg_clip_coef(const double* slots, int count, float grad_scale, float max_norm, float* record, int64_t* skipped, void* stream);
int dlsg_adam_clipped(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, int step,
                      float grad_scale, const float* hyper, const int32_t* guard, const float* record, float clip_value, void* stream);

/* ---------------------------------------------------------------- weight decay and an averaged copy of the weights, in Adam's pass
 * dlsg_adamw_ema: dlsg_adam_clipped with two further terms, per element and in torch's order:
 *   gi = (g * grad_scale) * record[DLSG_CLIP_COEF], clamped to +-clip_value when clip_value > 0       (dlsg_adam_clipped)
 *   decoupled == 0 (torch.optim.Adam(weight_decay=)):  gi += weight_decay * p     -- behind the clip: the record's norm has no decay term
 *   decoupled != 0 (torch.optim.AdamW):                p *= 1 - lr * weight_decay -- the plain lr, in front of the update
 *   m, v, p: dlsg_adam's update
 *   ema (optional, device, laid out as p): ema += (1 - ema_decay) * (p_new - ema)                    (torch.lerp, small weight)
 * hyper (optional, device) is FOUR floats here: {lr / (1 - b1^step), sqrt(1 - b2^step), the decay factor (1 - lr * weight_decay when
 *   decoupled, else weight_decay), 1 - ema_decay}, each computed in float64 and rounded once; without it the kernel takes the same
 *   four from its scalar arguments.  weight_decay == 0 compiles the decay out (hyper[2] is then not read), ema == NULL the average.
 * decay_ranges (optional, device): n_ranges <= DLSG_ADAM_MAX_RANGES intervals [lo, hi) as (n_ranges, 2) int64, in elements relative
 *   to p, sorted and disjoint, ends at any element: only elements inside one are decayed.  NULL / 0: the whole launch is decayed.
 *   The table is staged in LDS (16 B per interval) and searched by bisection once per 16-byte group.
 * guard != 0 or record[DLSG_CLIP_NONFINITE] != 0: p, m, v AND ema keep their bits.  p, g, m, v, ema at any float offset that they
 *   share; m, v, g and ema stream non-temporally, p does not (the next forward reads it).
 * With weight_decay == 0 and ema == NULL the launch is dlsg_adam_clipped's kernel: the same bits.
 * dlsg_swap_f32: a[i] <-> b[i] for i < n, in place (the weights against their average: addresses, and every captured graph that
 *   holds them, stay valid). */
#define DLSG_ADAM_MAX_RANGES 1024
int dlsg_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float b1, float b2, float eps,
                   int step, float grad_scale, float weight_decay, int decoupled, float ema_decay, const float* hyper,
                   const int32_t* guard, const float* record, float clip_value, const int64_t* decay_ranges, int n_ranges, void* stream);
int dlsg_swap_f32(float* a, float* b, int64_t n, void* stream);


/* ---------------------------------------------------------------- persistent BiLSTM recurrence (csrc/bilstm.hip)
 * Replaces the time loop of `nn.LSTM(H, H, bidirectional=True, batch_first=True)` in EncoderVisual (models/layer.py:26,52)
 * once the input half of the gates xg = e W_ih^T is known for all steps: ONE launch runs all T steps of both directions,
 * 2 * H/8 workgroups (one per CU, all resident), each keeping its 32 x H slice of W_hh in LDS and its cell states in
 * registers; h_t travels between workgroups through `hx` with write-through stores and per-step flags.
 * Layouts: xg[d] (B*T, >= 4H) rows b*T + t, gate order i,f,g,o (PyTorch); out (B, T, 2H) with direction d in columns
 * [dH, (d+1)H); hprev[d] (B, T, H) = h of the PREVIOUS step of direction d at each time index (the caller zero-fills it: the
 * first step of a direction is never written); c[d] (B, T, H); gates[d] (B, T, 4H) activated gates (what the backward reads).
 * Scratch owned by the caller: hx = dlsg_bilstm_hx_floats(T, H) floats, flags = dlsg_bilstm_flag_words(T, H) 32-bit words
 * (zeroed by the call itself), err = optional int32 that is set to 1 if a workgroup timed out waiting for another (the result
 * is then invalid; the device is never left spinning).  dlsg_bilstm_supported: B <= 64, H in {64, 512, 1024} and the current
 * device has at least 2 * H/8 compute units (all workgroups must be resident together). */
typedef struct {
    const float* xg[2];
    int64_t ldxg;
    const float* w_hh[2];
    const float* b_ih[2];
    const float* b_hh[2];
    float* out;
    float* hprev[2];
    float* c[2];
    float* gates[2];
    float* hx;
    uint32_t* flags;
    int32_t* err;
    int32_t B, T, H, pad_;
} dlsg_bilstm_args;
int dlsg_bilstm_supported(int B, int T, int H);
int64_t dlsg_bilstm_hx_floats(int T, int H);
int64_t dlsg_bilstm_flag_words(int T, int H);
int dlsg_bilstm_fwd(const dlsg_bilstm_args* a, void* stream);
/* Backward through time of the same recurrence, again ONE launch: from the saved activated gates / cell states and
 * dout (B, T, 2H) = d loss / d out, writes dgates[d] (B, T, 4H) = d loss / d (gate pre-activations) for every step (what the
 * weight / input gradient products after the loop contract).  Scratch: gx, px = dlsg_bilstm_bwd_x_floats(T, H) floats each
 * (per-step exchange of dG and of the K-quarter partials of dh), flags = 2 * dlsg_bilstm_flag_words(T, H) words. */
typedef struct {
    const float* gates[2];
    const float* c[2];
    const float* dout;
    const float* w_hh[2];
    float* dgates[2];
    float* gx;
    float* px;
    uint32_t* flags;
    int32_t* err;
    int32_t B, T, H, pad_;
} dlsg_bilstm_bwd_args;
int64_t dlsg_bilstm_bwd_x_floats(int T, int H);
int dlsg_bilstm_bwd(const dlsg_bilstm_bwd_args* a, void* stream);

/* ---------------------------------------------------------------- DiscV2's LSTM, a whole sequence per launch
 * Replaces `self.lstm = nn.LSTM(512, 512, batch_first=True)` of DiscV2 (models/model.py:122,139) inside a WGAN-GP critic
 * update (run_gun.py:352-371), where autograd differentiates it twice: level 0 = the forward recurrence, level 1 = its
 * backward through time (with the extra gradient inputs the gradient penalty's graph feeds in), level 2 = the backward of
 * that backward.  One persistent launch per level for all L steps (csrc/critic_lstm.hip; the per-step forms are
 * cell formulas in that file's header).  Tensors are contiguous, time-major (L, n, .) or batch-major (n, L, .) (`batch_major`):
 * gate tensors 4H wide (gate order i, f, g, o), states H wide.  n <= 256, H in {64, 512}; W = weight_hh (4H, H).
 *   level 0: addend = x W_ih^T + b_ih + b_hh  ->  As (pre-activations), Hs, Cs
 *   level 1: As, Cs, dHs, optional dAs / dCs  ->  DA (d As, injections included), DH, DC (total gradients reaching h_t, c_t)
 *   level 2: As, Cs, DH, DC, addend = gradient w.r.t. DA  ->  addend_out = Ubar (gradient w.r.t. dAs; optional, may alias addend),
 *            gA, gC (its last step is zero), gDH (gradient w.r.t. dHs), gDC (w.r.t. dCs)
 * xbuf / xbuf2: dlsg_lstm_seq_x_floats floats each (xbuf2 only at level 1), 16-byte aligned; flags: dlsg_lstm_seq_flag_words
 * words, zeroed by the call; err (optional): set non-zero if a workgroup timed out waiting (result then invalid). */
typedef struct {
    const float* addend;
    float* addend_out;
    const float* W;
    float* As; float* Hs; float* Cs;                 /* level 0 writes, levels 1-2 read As, Cs */
    const float* dHs; const float* dAs; const float* dCs;
    float* DA; float* DH; float* DC;                 /* level 1 writes, level 2 reads DH, DC */
    float* gA; float* gC; float* gDH; float* gDC;
    float* xbuf; float* xbuf2;
    uint32_t* flags;
    int32_t* err;
    int32_t L, n, H;
    int32_t batch_major;                             /* 0: (L, n, .) arrays; 1: (n, L, .) -- a sequence's steps are consecutive rows */
    const float* b_ih; const float* b_hh;            /* level 0, optional (both or neither): added to the addend */
    float* Hprev;                                    /* level 0, optional: Hprev_t = h_{t-1} (zeros at t = 0), layout of Hs */
    float* gDHprev;                                  /* level 2, optional: gDHprev_t = gDH_{t-1} */
} dlsg_lstm_seq_args;
int dlsg_lstm_seq_supported(int L, int n, int H);
int64_t dlsg_lstm_seq_x_floats(int L, int n, int H);
int64_t dlsg_lstm_seq_flag_words(int L, int n, int H);
int dlsg_lstm_seq(const dlsg_lstm_seq_args* a, int level, void* stream);

/* ---------------------------------------------------------------- gradient all-reduce over RCCL / xGMI
 * Replaces the gradient exchange of `DistributedDataParallel(model, find_unused_parameters=True)` over NCCL
 * (run_gun.py:63-64, train_debug.py:20): one process per GPU, sum of ranges of the flat gradient arena over all ranks,
 * in place; the mean (1/world) is folded into dlsg_adam's grad_scale.  librccl is resolved at run time (the instance a
 * PyTorch process has already mapped is reused), so the library loads without it; these calls then return DLSG_ENOCOMM.
 *
 * The communicator handle is the ONLY state the library keeps and the caller owns it:
 *   rank 0: dlsg_comm_unique_id(id)  ->  the caller ships the 128 bytes to every rank (any side channel: torch.distributed
 *   store, MPI, a file)  ->  every rank, with its device current: dlsg_comm_init(&c, id, world, rank) (collective)
 *   ...  dlsg_allreduce_bucket(c, grads + lo, hi - lo, stream) per gradient bucket, same order on every rank  ...
 *   dlsg_comm_destroy(c).
 * The collectives are asynchronous on `stream` and may be stream-captured: dlsg_amd.Trainer forks a side stream inside the
 * capture of the train step, so the bucket all-reduces overlap the remaining backward within ONE replayed hipGraph. */
#define DLSG_COMM_ID_BYTES 128
typedef struct dlsg_comm dlsg_comm;
int dlsg_comm_unique_id(void* id128);
int dlsg_comm_init(dlsg_comm** out, const void* id128, int world, int rank);
int dlsg_comm_destroy(dlsg_comm* c);
int dlsg_comm_info(const dlsg_comm* c, int32_t* world, int32_t* rank, int32_t* rccl_version);
int dlsg_allreduce_bucket(dlsg_comm* c, float* grads, int64_t count, void* stream);
/* n ranges of one bucket as one RCCL group (one fused launch) */
int dlsg_allreduce_buckets(dlsg_comm* c, float* const* grads, const int64_t* counts, int n, void* stream);
/* words[i] <- max over the ranks (int32), on `stream`: the persistent kernels' time-out word travels with the first gradient
 * bucket, so that dlsg_adam's guard skips the update on EVERY rank or on none. */
int dlsg_allreduce_max_i32(dlsg_comm* c, int32_t* words, int64_t count, void* stream);
/* Rehearsal instrument for one-GPU boxes (with one rank an all-reduce moves nothing): `workgroups` x 256 threads -- RCCL's launch
 * shape -- stream buf[0..count) `passes` times, read-modify-write with a factor of 1.0f (values unchanged), on `stream`: the
 * CUs and the HBM share a bucket's ring all-reduce would hold while the backward runs beside it.  No communicator involved;
 * buf 16-B aligned. */
int dlsg_comm_rehearsal(float* buf, int64_t count, int workgroups, int passes, void* stream);
/* *code <- ncclCommGetAsyncError of the communicator (0 = no error); does not synchronise. */
int dlsg_comm_async_error(dlsg_comm* c, int32_t* code);

#ifdef __cplusplus
}
#endif
#endif
