/*
 * csu.h -- C ABI of libcsu_hip.so, the MI355X (gfx950) kernels of the CSWin-(SimAM-)UNet
 * training path.  Plain pointers, int sizes and a hipStream_t passed as void*; no framework
 * types.  Every buffer is owned by the caller (the library never allocates); every call is
 * asynchronous on `stream` and reentrant.  Return 0 on success, a positive hipError_t, or a
 * negative CSU_E* code; csu_last_error_string() describes the last failure of the calling thread.
 *
 * Layout convention: activations are token-major "(B, L, C)" = NHWC with L = H*W, exactly the
 * reference's token layout (train_cswinunet_segmentation.py, the `B, L, C` tensors of
 * cswin:349-370), so no NCHW transposes are needed between ops.
 *
 * The reference has no FFI (it is pure PyTorch); each entry point below names the reference
 * operator it replaces (cswin:N = train_cswinunet_segmentation.py line N,
 * unet:N = train_unet_segmentation.py line N).  The Python binding is csu/_lib.py (ctypes).
 */
#ifndef CSU_H_
#define CSU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum csu_dtype { CSU_F32 = 0, CSU_BF16 = 1 };

enum csu_status {
    CSU_OK = 0,
    CSU_E_ARG = -1,       /* invalid argument (shape, dtype, null pointer) */
    CSU_E_UNSUPPORTED = -2,
    CSU_E_WORKSPACE = -3  /* workspace too small */
};

const char* csu_last_error_string(void);
/* Library version and the offload arch it was built for ("gfx950"). */
const char* csu_build_info(void);

/* Timing events for bench.py's per-kernel roofline ledger (measurement plumbing, not part of the
 * reference interface).  csu_event_record_ext: inside a stream capture it appends an event-record
 * NODE to the graph being captured (hipGraphAddEventRecordNode after the stream's current
 * dependencies, which it then replaces), so every replay re-stamps it and csu_event_elapsed_ms
 * gives each captured kernel's time in that replay (torch refuses external events on ROCm).
 * Outside a capture it is a plain hipEventRecord. */
int csu_event_create(void** event);
int csu_event_destroy(void* event);
int csu_event_record_ext(void* event, void* stream);
int csu_event_elapsed_ms(void* start, void* end, float* ms);

/* ---------------------------------------------------------------------------------------
 * Cross-shaped stripe attention with LePE (LePEAttention.forward, cswin:271-298, geometry
 * cswin:232-240, get_v depthwise 3x3 cswin:244/256-269; branch split + concat of
 * CSWinBlock.forward cswin:358-363).  One call runs every branch of a CSWinBlock: branch i
 * reads its Q/K/V channels [ch_off, ch_off + heads*head_dim) of the (B, L, 3C) qkv Linear
 * output and writes the same channels of the (B, L, C) output (the torch.cat is free).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int32_t H_sp, W_sp;      /* stripe window: idx0 (reso, sw), idx1 (sw, reso), idx-1 (reso, reso) */
    int32_t ch_off;          /* first channel of this branch inside C (0 or C/2) */
    int32_t _pad;
    const float* lepe_w;     /* get_v.weight (C_b, 1, 3, 3), fp32 master weight */
    const float* lepe_b;     /* get_v.bias (C_b), fp32 */
    float* lepe_dw;          /* backward: written (not accumulated) gradient of lepe_w */
    float* lepe_db;          /* backward: gradient of lepe_b */
} csu_stripe_branch;

typedef struct {
    int32_t B, reso, C;      /* L = reso*reso tokens; qkv rows are 3C wide, output rows C wide */
    int32_t heads;           /* heads per branch (num_heads/2, or num_heads for the last stage) */
    int32_t head_dim;        /* must be 32 (embed_dim is hard-wired to 64: SURVEY §0.5) */
    int32_t nbranch;         /* 1 (last stage, idx -1) or 2 (idx 0 and idx 1) */
    float scale;             /* qk_scale or head_dim**-0.5 (cswin:231) */
    int32_t split;           /* workgroups per window-head of the whole-window bf16 kernels: 0 = the
                              * heuristic, 1 .. ceil(roundup32(N) / 128) forces that factor (tests,
                              * tuning).  The range is checked in every call and dtype (anything else is
                              * CSU_E_ARG, so the field must be initialised: it was padding before); the
                              * value is used only where a whole-window bf16 kernel runs */
    csu_stripe_branch br[2];
    /* attention dropout on the softmax probabilities (attn_drop, cswin:290), p = 0: none.  rng =
     * device [seed, counter] snapshot of the step (uint64 x 2), the same for forward and backward;
     * branch i uses dropout site drop_site + i.  Mask element of (branch, image b, window win,
     * head hh, query q, key k): ((((b * nwin + win) * heads + hh) * N + q) * Npad + k) with
     * N = window tokens, Npad = N rounded up to 32 (csu_dropout_mask materialises it). */
    const uint64_t* drop_rng;
    uint32_t drop_site;
    float drop_p;
} csu_stripe_args;

/* out (B, L, C) dtype; lse fp32 [nbranch][B][heads][L] (softmax log-sum-exp, saved for bwd). */
int csu_stripe_attn_fwd(const csu_stripe_args* a, int dtype, const void* qkv, void* out,
                        float* lse, void* stream);

/* Workspace bytes csu_stripe_attn_bwd needs (fp32 partial sums of the LePE weight gradient). */
size_t csu_stripe_attn_bwd_workspace(const csu_stripe_args* a);

/* Gradient of the forward above.  out = forward output, dout = its gradient (B, L, C);
 * delta fp32 scratch shaped like lse; dqkv (B, L, 3C) is fully written (Q|K|V slots of every
 * branch's channels); lepe_dw / lepe_db of each branch are written. */
int csu_stripe_attn_bwd(const csu_stripe_args* a, int dtype, const void* qkv, const void* out,
                        const void* dout, const float* lse, float* delta, void* dqkv,
                        void* workspace, size_t workspace_bytes, void* stream);
/* LePE weight/bias gradient alone (csu_stripe_attn_bwd skips it when every lepe_dw / lepe_db of
 * the args is NULL): lets it run on a second stream, concurrently with the dQ / dK / dV kernels.
 * Workspace: csu_stripe_attn_bwd_workspace bytes. */
int csu_stripe_lepe_wgrad(const csu_stripe_args* a, int dtype, const void* qkv, const void* dout,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Deferred LePE weight gradient: csu_stripe_attn_bwd_ex with lepe_deferred = 1 leaves the per-block
 * partials in `workspace` (csu_stripe_lepe_nblk(a, dtype) blocks) instead of reducing them; one
 * csu_stripe_lepe_reduce_batch launch later reduces many such workspaces (e.g. every block's at the
 * end of a backward pass).  channels = heads * 32 per branch; dw [channels][9], db [channels]. */
int csu_stripe_attn_bwd_ex(const csu_stripe_args* a, int dtype, const void* qkv, const void* out, const void* dout,
                           const float* lse, float* delta, void* dqkv, void* workspace, size_t workspace_bytes,
                           int lepe_deferred, void* stream);
int csu_stripe_lepe_nblk(const csu_stripe_args* a, int dtype);
typedef struct {
    const float* part;
    float* dw[2];
    float* db[2];
    int32_t nblk, channels, nbranch, _pad;
} csu_lepe_reduce_item;
int csu_stripe_lepe_reduce_batch(const csu_lepe_reduce_item* items, int count, void* stream);

/* The launch plan of a stripe-attention call: which kernel instance csu_stripe_attn_fwd /
 * csu_stripe_attn_bwd(_ex) / csu_stripe_lepe_wgrad run for (args, dtype) and how each divides the
 * window.  Host only, no HIP call: it is the function the launch layer itself takes every decision
 * from, so the report cannot differ from what is launched. */
enum csu_stripe_kernel {
    CSU_STRIPE_STREAMED = 0,      /* stripe_fwd / stripe_bwd_dq + _dkdv: one workgroup per 128-row block */
    CSU_STRIPE_WINDOW = 1,        /* stripe_fwd_w / stripe_bwd_dq_w + _dkdv_w: whole window in LDS, split */
    CSU_STRIPE_FUSED_BWD = 2      /* stripe_bwd_fused_w: one-pass backward, one workgroup per window-head */
};
enum csu_lepe_kernel {
    CSU_LEPE_IN_FUSED_BWD = 0,    /* pass 1 (block partials) formed inside stripe_bwd_fused_w */
    CSU_LEPE_TILES = 1,           /* lepe_wgrad_tiles */
    CSU_LEPE_PARTIAL = 2          /* lepe_wgrad_partial */
};
enum csu_stripe_plan_flags {
    CSU_PLAN_RAGGED_PASS = 1,     /* a workgroup's last of several passes has idle waves */
    CSU_PLAN_EMPTY_PARTNER = 2    /* a split partner owns no rows (its first row is at or past the padded
                                   * window's end): odd splits only, e.g. sp 7 for windows of 897..960 tokens */
};
typedef struct {
    int32_t kernel;               /* csu_stripe_kernel */
    int32_t wm;                   /* LDS image rows of the instance (WINDOW, FUSED_BWD), else 0 */
    int32_t sp;                   /* split factor chosen (args.split or the heuristic); 1 where no split kernel runs */
    int32_t split;                /* workgroups per window-head as launched (sp, or sp / 2 with 8 waves;
                                   * STREAMED: the 128-row blocks of the window) */
    int32_t waves;                /* waves per workgroup */
    int32_t rows;                 /* rows a workgroup owns (STREAMED: 128; FUSED_BWD: wm) */
    int32_t passes;               /* most passes of 32 * waves rows a wave makes over its workgroup's rows
                                   * (FUSED_BWD: key tiles per wave) */
    int32_t flags;                /* csu_stripe_plan_flags */
} csu_stripe_kernel_plan;
typedef struct {
    csu_stripe_kernel_plan fwd, bwd;
    int32_t lepe_kernel;          /* csu_lepe_kernel: where pass 1 of csu_stripe_attn_bwd's LePE weight gradient runs */
    int32_t lepe_nblk;            /* block partials it leaves (csu_stripe_lepe_nblk) */
    /* the stand-alone pass 1 (csu_stripe_lepe_wgrad; the backward's too unless IN_FUSED_BWD) */
    int32_t wgrad_kernel;         /* CSU_LEPE_TILES or CSU_LEPE_PARTIAL */
    int32_t wgrad_nblk;           /* its block partials per branch */
    int32_t tile_rows;            /* TILES: image rows per tile, rows per block, tiles per block (PARTIAL: 0) */
    int32_t rows_blk;
    int32_t tiles_blk;
    int32_t wgrad_flags;          /* TILES: 1 = an image's last block has fewer rows than rows_blk,
                                   *        2 = a block's last tile reaches past the block's rows */
    int32_t ws_blocks;            /* partial blocks per branch the workspace is sized for (either dtype) */
    int32_t _pad;
} csu_stripe_plan;
/* Runs the same validation as the launches; 0 or a csu_status. */
int csu_stripe_attn_plan(const csu_stripe_args* a, int dtype, csu_stripe_plan* out);

/* ---------------------------------------------------------------------------------------
 * LayerNorm over the last dim C of (rows, C) (nn.LayerNorm: norm1/norm2 cswin:315/347,
 * Merge_Block.norm cswin:377, patch-embed LN cswin:507, norm/norm_up cswin:554/602).
 * x dtype = xdtype, y dtype = ydtype (bf16 output feeds the next GEMM directly), gamma/beta
 * fp32; mean/rstd fp32 [rows] are saved for backward.
 * ------------------------------------------------------------------------------------- */
int csu_layernorm_fwd(int rows, int C, float eps, int xdtype, const void* x, const float* gamma,
                      const float* beta, int ydtype, void* y, float* mean, float* rstd, void* stream);
size_t csu_layernorm_bwd_workspace(int rows, int C);
/* dx (xdtype) written; dgamma/dbeta fp32 written (deterministic two-pass reduction). */
int csu_layernorm_bwd(int rows, int C, int xdtype, const void* x, const float* gamma,
                      const float* mean, const float* rstd, int dydtype, const void* dy,
                      void* dx, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes,
                      void* stream);
/* Residual-junction backward of y = LN(x) inside x_out = x + f(y) (CSWinBlock cswin:367-368):
 * dx = dres + dLN(dy) in one pass (dres fp32 [rows][C] or NULL; x/dx fp32 when dres is given),
 * plus an optional bf16 copy dx_bf16 (the next GEMM's operand; NULL to skip).  Replaces the
 * autograd add of the two branches and the bf16 cast of the summed gradient. */
int csu_layernorm_bwd_ex(int rows, int C, int xdtype, const void* x, const float* gamma,
                         const float* mean, const float* rstd, int dydtype, const void* dy,
                         const float* dres, void* dx, void* dx_bf16, float* dgamma, float* dbeta,
                         void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * SimAM (parameter-free energy gate) on token rows (B, L, C), statistics per (b, c) over L.
 * NOT in the reference: public SimAM formula; parity unpinned vs the
 * reference.  stats fp32 [B][C][2] = (mean, 4*(var_unbiased + lambda)) saved for backward.
 * ------------------------------------------------------------------------------------- */
/* dgamma / dbeta from the per-block partials that csu_layernorm_bwd_ex left in `workspace` when
 * called with dgamma = dbeta = NULL (same rows / C): the parameter reduction can then run on a
 * second stream, off the input-gradient chain. */
int csu_layernorm_param_reduce(int rows, int C, const void* workspace, float* dgamma, float* dbeta, void* stream);
/* the same for many layers in one launch (the deferred end-of-backward reduction of every
 * LayerNorm's dgamma / dbeta): items is a HOST array, copied into the kernel arguments */
typedef struct {
    const void* workspace;
    float* dgamma;
    float* dbeta;
    int32_t rows, C;
    int32_t nblocks;   /* partial rows in the workspace; 0: those of csu_layernorm_bwd_ex for `rows` */
    int32_t _pad;
} csu_ln_param_item;
int csu_layernorm_param_reduce_batch(const csu_ln_param_item* items, int count, void* stream);

size_t csu_simam_workspace(int B, int L, int C);
/* y (ydtype, e.g. bf16 for the GEMM that consumes the gated skip) = SimAM(x); C % 4 == 0 */
int csu_simam_fwd(int B, int L, int C, float lambda, int xdtype, const void* x, int ydtype, void* y, float* stats,
                  void* workspace, size_t ws_bytes, void* stream);
/* dx (xdtype) from dy (gdtype) */
int csu_simam_bwd(int B, int L, int C, int xdtype, const void* x, const float* stats, int gdtype, const void* dy,
                  void* dx, void* workspace, size_t ws_bytes, void* stream);
/* The skip fork of the CSWin-SimAM-UNet encoder (an fp32 stage output feeding the Merge_Block conv
 * and, through SimAM, the decoder's concat_linear -- cswin:530-545 / 568-592 + the SimAM gate):
 * y = bf16(SimAM(x)) and xc = bf16(x) from the same passes (no separate cast of x). */
int csu_simam_fwd_fork(int B, int L, int C, float lambda, const float* x, void* y, void* xc, float* stats,
                       void* workspace, size_t ws_bytes, void* stream);
/* its backward: dx = g2 + (SimAM input gradient of dy), dxb = bf16(dx); g2 bf16 (the conv's input
 * gradient), dy gdtype -- the autograd sum and both casts in the gate-gradient pass */
int csu_simam_bwd_join(int B, int L, int C, const float* x, const float* stats, int gdtype, const void* dy,
                       const void* g2, float* dx, void* dxb, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * CARAFE content-aware reassembly (CARAFE/CARAFE4.forward cswin:401-437 / 450-486, from the
 * encoder logits to the input of the `out` 1x1 conv: pixel_shuffle + softmax over 9 taps +
 * unfold + (C x 9)@(9 x s^2) + pixel_shuffle, fused).  x (B, H*W, C) tokens, enc (B, H, W, 9*s*s)
 * NHWC logits with channel t*s*s + i*s + j, out (B, sH*sW, C); wsave fp32 (B, H, W, 9*s*s)
 * softmax weights written by fwd for bwd.  C = 8 * 2^k <= 512.
 * ------------------------------------------------------------------------------------- */
int csu_carafe_fwd(int B, int H, int W, int C, int s, int dtype, const void* x, const void* enc,
                   void* out, float* wsave, void* stream);
/* dx (B, H*W, C) and denc (B, H, W, 9*s*s) written. */
int csu_carafe_bwd(int B, int H, int W, int C, int s, int dtype, const void* x, const float* wsave,
                   const void* dout, void* dx, void* denc, void* stream);

/* ---------------------------------------------------------------------------------------
 * 1-class output head: 1x1 conv without bias + sigmoid (CSWinTransformer.up_x4 `output`
 * cswin:603/680 and forward's torch.sigmoid cswin:688).  x (P, C) tokens, w (C) fp32,
 * prob (P) fp32.  C in {8, 16, 32, 64}.
 * ------------------------------------------------------------------------------------- */
int csu_head_fwd(long P, int C, int dtype, const void* x, const float* w, float* prob, void* stream);
size_t csu_head_bwd_workspace(long P, int C);
/* dprob -> dx (P, C) and dw (C) (deterministic two-pass reduction). */
int csu_head_bwd(long P, int C, int dtype, const void* x, const float* w, const float* prob,
                 const float* dprob, void* dx, float* dw, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused CARAFE4 + 1-class output head (CSWinTransformer.up_x4 + sigmoid, cswin:674-688):
 * everything after upsample1's encoder conv is linear up to the sigmoid, so with
 * u = W_out^T w_output (C fp32) and cb = w_output . b_out (1 fp32, device), computed by the caller,
 *   prob[b, s y + i, s x + j] = sigmoid(sum_t m[t] z[nbr_t(y, x)] + cb),  z[q] = u . x[q]
 * (m = softmax over the 9 taps of enc[b, y, x, t*s*s + i*s + j]; cswin:456-481).  x (B, H*W, C)
 * tokens, enc NHWC (B, H, W, 9 s^2), z fp32 (B*H*W) written for bwd, prob fp32 (B, sH, sW).
 * s in {2, 4}; C = 8 * 2^k <= 512.
 * ------------------------------------------------------------------------------------- */
int csu_carafe_head_fwd(int B, int H, int W, int C, int s, int dtype, const void* x, const void* enc,
                        const float* u, const float* cb, float* z, float* prob, void* stream);
size_t csu_carafe_head_bwd_workspace(int B, int H, int W, int C, int s);
/* dprob -> dx (B, H*W, C), denc (B, H, W, 9 s^2), du (C) and dcb (1), fp32 reductions deterministic. */
int csu_carafe_head_bwd(int B, int H, int W, int C, int s, int dtype, const void* x, const void* enc,
                        const float* z, const float* u, const float* prob, const float* dprob, void* dx,
                        void* denc, float* du, float* dcb, void* workspace, size_t ws_bytes, void* stream);
/* Head-weight folding (the `out` 1x1 conv w_out (O x C) + b_out (O) and the 1-class `output` conv
 * w_h (O), cswin:674-688): u = w_out^T w_h, cb = w_h . b_out (fp32, one launch, fixed order). */
int csu_head_fold_fwd(int O, int C, const float* w_out, const float* b_out, const float* w_h, float* u, float* cb,
                      void* stream);
typedef struct {
    int32_t O;
    const float* w_out;  /* (O, C) */
    const float* b_out;  /* (O) */
    const float* w_h;    /* (O) */
    float* dw_out;       /* (O, C) = w_h du^T */
    float* db_out;       /* (O) = w_h dcb */
    float* dw_h;         /* (O) = w_out du + b_out dcb */
} csu_head_fold;
/* csu_carafe_head_bwd with the folding's backward appended (gradients of w_out, b_out, w_h from du
 * and dcb inside the same call; dcb itself not returned) */
int csu_carafe_head_bwd_fold(int B, int H, int W, int C, int s, int dtype, const void* x, const void* enc,
                             const float* z, const float* u, const float* prob, const float* dprob, void* dx,
                             void* denc, float* du, const csu_head_fold* fold, void* workspace, size_t ws_bytes,
                             void* stream);

/* ---------------------------------------------------------------------------------------
 * Deterministic column sum out[c] = sum_r in[r][c], fp32 accumulation (rows x cols row-major,
 * dtype in; out fp32).  The bias gradient of every nn.Linear (cswin:185/187/314/323/568/581/592)
 * is the column sum of dY over the B*L tokens; also reduces split-K weight-gradient slabs.
 * ------------------------------------------------------------------------------------- */
size_t csu_colsum_workspace(long rows, long cols, int dtype);
int csu_colsum(long rows, long cols, int dtype, const void* in, float* out, void* workspace,
               size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Linear weight + bias gradient over M token rows (backward of every nn.Linear on tokens:
 * cswin:185/187/314/323/568/581/592 and the CARAFE 1x1 convs cswin:396/399).
 * dy (M, N), x (M, K) row-major, dtype in; dw_db fp32 [N*K + N] = dW (N, K) then db (N), written.
 * Split-K over M with MFMA tiles; the chunk partials are summed in a fixed order (bitwise
 * reproducible).  N, K multiples of 16 bytes.
 * ------------------------------------------------------------------------------------- */
size_t csu_linear_wgrad_workspace(long M, int N, int K);
int csu_linear_wgrad(long M, int N, int K, int dtype, const void* dy, const void* x, float* dw_db,
                     void* workspace, size_t ws_bytes, void* stream);
/* Deferred form (bf16): only the tile kernel runs now; when the plan splits the tokens
 * (item->chunks > 1) the chunk partials stay in `workspace` and dw_db is written later by
 * csu_wslab_reduce_batch over the returned items (one launch for many Linears, e.g. at the end of
 * a backward pass; workspace and dw_db must stay allocated until then).  item->chunks == 1: dw_db
 * is already written. */
typedef struct {
    const float* slab;
    float* dst;
    int32_t N, K, tn, tk, chunks, _pad;
} csu_wslab_item;
int csu_linear_wgrad_deferred(long M, int N, int K, const void* dy, const void* x, float* dw_db,
                              void* workspace, size_t ws_bytes, csu_wslab_item* item, void* stream);
int csu_wslab_reduce_batch(const csu_wslab_item* items, int count, void* stream);
/* Grouped weight gradients (bf16): the tile kernels of many Linears in one launch per tile size
 * (items: HOST array, copied into kernel arguments, <= 48 items per launch).  Each item's plan
 * (tile, token chunks) comes from csu_linear_wgrad_group_plan, which returns the slab workspace
 * bytes the item needs (0: dw_db is written directly); items with chunks > 1 are completed by
 * csu_wslab_reduce_batch with {slab, dw_db, N, K, tn, tk, chunks}.  M < 2^31 tokens. */
typedef struct {
    const void* dy;      /* (M, N) bf16 */
    const void* x;       /* (M, K) bf16 */
    float* dw_db;        /* N*K + N fp32 */
    float* slab;         /* workspace of csu_linear_wgrad_group_plan's size, or NULL if 0 */
    int64_t M;
    int32_t N, K;
} csu_wgrad_group_item;
size_t csu_linear_wgrad_group_plan(long M, int N, int K, int* tn, int* tk, int* chunks);
int csu_linear_wgrad_group(const csu_wgrad_group_item* items, int count, void* stream);
/* The same launches planned over the whole list: one common target chunk length per launch, so
 * that the workgroups of a launch fill whole rounds of the CUs (csu_linear_wgrad_group_plan cuts
 * each Linear alone).  plan_all reads M, N, K and the order of the items only (never the
 * pointers); cus = 0 asks the device, cus > 0 makes no GPU call.  The plan is a function of
 * (cus, shapes in order) alone.  Per item: the tile (csu_linear_wgrad_group_plan's), the token
 * chunks, rows per chunk (a multiple of 64; the last chunk may be shorter), the slab workspace the
 * item needs (0: dw_db is written directly; <= operand bytes / 8), the launch it goes to (launches
 * run in ascending order, <= 48 items each, one tile shape) and its position in that launch.
 * csu_linear_wgrad_group_planned launches items with such plans (slab: plan's slab_bytes); items
 * with chunks > 1 are completed by csu_wslab_reduce_batch as above.  csu_linear_wgrad_group_model:
 * the constants of the dispatch model the plan minimises (us per workgroup = fixed + 64-token steps
 * x step; workgroups resident per CU). */
typedef struct {
    int32_t tn, tk, chunks, launch, pos, _pad;
    int64_t rpc;
    uint64_t slab_bytes;
} csu_wgrad_group_plan;
int csu_linear_wgrad_group_plan_all(const csu_wgrad_group_item* items, int count, int cus, csu_wgrad_group_plan* out);
int csu_linear_wgrad_group_planned(const csu_wgrad_group_item* items, const csu_wgrad_group_plan* plans, int count,
                                   void* stream);
void csu_linear_wgrad_group_model(int tn, int tk, double* fixed_us, double* step_us, int* wg_per_cu);
/* Same with the plan forced (tuning / tests): bf16 output tile tn x tk (64 or 128; 0 = auto) and
 * the number of token chunks (0 = auto).  The fp32 path ignores them. */
size_t csu_linear_wgrad_tuned_workspace(long M, int N, int K, int tn, int tk, int chunks);
int csu_linear_wgrad_tuned(long M, int N, int K, int dtype, const void* dy, const void* x, float* dw_db,
                           void* workspace, size_t ws_bytes, int tn, int tk, int chunks, void* stream);

/* ---------------------------------------------------------------------------------------
 * Token GEMM, bf16 operands, fp32 accumulation, fused prologue/epilogue (nn.Linear of
 * CSWinBlock/Mlp cswin:185-195, 314-368 plus the GELU, GELU-backward and residual-add passes):
 *   out[m][n] = ((sum_k pro(a[m][k]) * B(n,k)) + bias[n]) * gelu'(gelu_aux[m][n]) + resid[m][n]
 *   B(n,k) = b[n*ldb + k] (b_trans = 0) or b[k*ldb + n] (b_trans = 1); pro = gelu if a_gelu.
 * bias / gelu_aux (bf16, ld = ldc) / resid (fp32, ld = ldc) may be NULL; resid needs out fp32.
 * K, lda, ldb multiples of 8 (and N when b_trans).
 * ------------------------------------------------------------------------------------- */
int csu_gemm(long M, int N, int K, const void* a, int lda, const void* b, int ldb, int b_trans, int a_gelu,
             const float* bias, const void* gelu_aux, const float* resid, void* out, int ldc, int out_dtype,
             void* stream);
/* Extended form: everything csu_gemm takes plus
 *   gelu_out  bf16 (M, ldc) or NULL: also write gelu(out) (exact erf GELU) -- fc1's activation
 *             next to its pre-activation (needs out bf16, no gelu_aux/resid);
 *   cfg       tile configuration of the b_trans = 0 kernel (0: 64x64, 1: 64x128, 2: 128x64,
 *             3: 128x128; -1 = per-shape choice, what csu_gemm uses). */
typedef struct {
    int64_t M;
    int32_t N, K;
    const void* a;
    const void* b;
    int32_t lda, ldb;
    int32_t b_trans, a_gelu;
    const float* bias;
    const void* gelu_aux;
    const float* resid;
    void* out;
    void* gelu_out;
    int32_t ldc, out_dtype;
    int32_t cfg, _pad;
} csu_gemm_desc;
int csu_gemm_ex(const csu_gemm_desc* d, void* stream);

/* The proj Linear + residual of CSWinBlock (cswin:366-367, K = N = C in {64, 128, 256}) with the
 * block's norm2 LayerNorm (cswin:368 -> Mlp input) in the epilogue: out = resid + x W^T + bias (fp32,
 * as csu_gemm_ws with resid) and ln_out = bf16(LayerNorm(out; gamma, beta, eps)) + the per-token mean /
 * rstd (fp32) for its backward.  M % (64 or 128) == 0 (csu_gemm_ws_ln_supported). */
int csu_gemm_ws_ln_supported(long M, int C, int K);
int csu_gemm_ws_ln(long M, int C, const void* x, int ldx, const void* w_frag, const float* bias, const float* resid,
                   float* out, const float* gamma, const float* beta, float eps, void* ln_out, float* mean, float* rstd,
                   void* stream);

/* ---------------------------------------------------------------------------------------
 * Weight-streaming token GEMM (csrc/gemm_ws.hip): out (M, N) = x (M, K) @ W^T (+ bias) (+ resid),
 * for the CSWinBlock qkv / proj Linears (cswin:337, 366) and their input gradients at C = 128 / 256.
 * x bf16 with row stride ldx; w_frag = W (N, K) bf16 in FRAGMENT order (csu_frag_layout_batch);
 * bias fp32 (N) or NULL; resid fp32 (M, N) or NULL (then out_dtype must be CSU_F32); out_dtype
 * CSU_BF16 or CSU_F32, out (M, N) contiguous.  csu_gemm_ws_supported says whether (M, N, K, resid,
 * out_dtype) is instantiated (M % 64 == 0; (K, N) in {(128,384), (256,768), (384,128), (768,256),
 * (128,128), (256,256)}); other shapes return CSU_E_ARG.
 * ------------------------------------------------------------------------------------- */
int csu_gemm_ws_supported(long M, int N, int K, int resid, int out_dtype);
int csu_gemm_ws(long M, int N, int K, const void* x, int ldx, const void* w_frag, const float* bias, const float* resid,
                int out_dtype, void* out, void* stream);
/* The input gradient of a LayerNorm -> Linear pair (CSWinBlock norm1 -> qkv, cswin:357 / 337) with the
 * LayerNorm backward in the GEMM's epilogue: dh = dy (M, K) @ W^T-fragments (wt_frag: the (C, K) weight
 * transpose, fragment-ordered) is never written -- it is rounded to bf16 as csu_gemm_ws would store it
 * and consumed in the kernel; instead dx (M, C) fp32 = dres + rstd (g - mean(g) -
 * xhat mean(g xhat)), g = dh * gamma, xhat = (x - mean) rstd, its bf16 copy dx_bf16, and the dgamma /
 * dbeta column partials of every 64-token block into part [M / 64][2C] (reduce them with
 * csu_layernorm_param_reduce_batch, nblocks = M / 64).  x fp32 (M, C); dres fp32 (M, C) or NULL.
 * Instantiated for (C, K) = (128, 384), (256, 768); M % 64 == 0 (csu_gemm_ws_lnbwd_supported). */
int csu_gemm_ws_lnbwd_supported(long M, int C, int K);
int csu_gemm_ws_lnbwd(long M, int C, int K, const void* dy, const void* wt_frag, const float* x, const float* gamma,
                      const float* mean, const float* rstd, const float* dres, float* dx, void* dx_bf16, float* part,
                      void* stream);
/* Fragment-ordered copy of a bf16 (rows x cols) matrix, rows % 32 == 0, cols % 16 == 0: 16-B chunk
 * q of row n (k = 8q .. 8q+7) goes to chunk ((n / 32) * (cols / 16) + q / 2) * 64 + n % 32 + 32 (q % 2),
 * i.e. [rows/32][cols/16][64 lanes][8] -- the MFMA 32x32x16 A-operand fragment of lane (n % 32, half).
 * items: DEVICE array sorted by chunk0 (first 16-B chunk of the item; chunk0[i+1] = chunk0[i] +
 * rows * cols / 8); total_chunks = the sum. */
typedef struct {
    const void* src;
    void* dst;
    int32_t rows, cols;
    int64_t chunk0;
} csu_frag_item;
int csu_frag_layout_batch(const csu_frag_item* items, int count, long total_chunks, void* stream);

/* e4m3 weights (BASELINE config 5, the fp8 format's qkv / proj Linears): csu_gemm_ws with W = q * s[n]
 * given as e4m3 bytes q in fragment order (csu_frag8_layout_batch: [N/32][K/16][64 lanes][8 bytes]) and
 * per-row power-of-two scales s (fp32, length N of the Linear).  scale_mode 1: out = x W^T (w_frag8 =
 * the fragments of q, s indexed by the output column); 2: out = dy W, the input gradient (w_frag8 = the
 * fragments of q^T, s indexed by the reduction index).  Bitwise equal to csu_gemm_ws on the dequantised
 * bf16 weight (power-of-two scales are applied exactly); same shapes / epilogues as csu_gemm_ws.
 * csu_gemm_ws_ln_e4m3: csu_gemm_ws_ln with e4m3 weights (scale_mode 1). */
int csu_gemm_ws_e4m3(long M, int N, int K, const void* x, int ldx, const void* w_frag8, const float* w_scale,
                     int scale_mode, const float* bias, const float* resid, int out_dtype, void* out, void* stream);
int csu_gemm_ws_ln_e4m3(long M, int C, const void* x, int ldx, const void* w_frag8, const float* w_scale,
                        const float* bias, const float* resid, float* out, const float* gamma, const float* beta,
                        float eps, void* ln_out, float* mean, float* rstd, void* stream);
/* e4m3 fragment order of an e4m3 (N x K) matrix src (transpose 0: of src itself, rows N; 1: of src^T,
 * rows K); N % 32 == 0, K % 32 == 0.  items: DEVICE array sorted by block0, the first 8x8-byte source
 * block of the item (block0[i+1] = block0[i] + N * K / 64); total_blocks = the sum. */
typedef struct {
    const void* src;
    void* dst;
    int32_t N, K;
    int32_t transpose, _pad;
    int64_t block0;
} csu_frag8_item;
int csu_frag8_layout_batch(const csu_frag8_item* items, int count, long total_blocks, void* stream);

/* ---------------------------------------------------------------------------------------
 * Batched weight cast: for each item, dst (rows, cols) bf16 = src fp32, and when dst_t is not
 * NULL also dst_t (cols, rows) bf16 = src^T.  items is a DEVICE array sorted by tile0, the first
 * 64x64-tile index of the item (tile0[i+1] = tile0[i] + ceil(rows/64) * ceil(cols/64));
 * total_tiles = the sum.  One launch per step refreshes every bf16 shadow weight.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* src;
    void* dst;
    void* dst_t;
    int32_t rows, cols;
    int64_t tile0;
    int32_t taps;   /* 0: matrix item.  > 0: conv weight src (rows=N, cols=C, taps=KH*KW) -> dst = OHWI
                       [N][KH][KW][C], dst_t = IHWO [C][KH][KW][N] (or NULL); ceil(N*C*taps/4096) tiles */
    int32_t cols_pad;   /* conv items: channel stride of dst (0 = C; > C: channel-padded OHWI whose
                           pad channels are left untouched, e.g. zeroed once by the caller) */
} csu_cast_item;
int csu_cast_bf16_batch(const csu_cast_item* items, int count, long total_tiles, void* stream);

/* fp8-e4m3 weights (BASELINE config 5): per item (rows x cols fp32 row-major, row = output feature),
 * per row the power-of-two scale s = 2^ceil(log2(amax/448)) -- the smallest power of two with amax / s <= 448,
 * taken exactly from the float's exponent and mantissa (e4m3_row_scale, csrc/common.hpp), never through an fp32
 * log2 --, q = e4m3fn(w / s) (RNE), and
 * dst = q * s in fp32 (exact in bf16: the cast cache then makes the kernels' bf16 shadows from it);
 * dst_q (optional) the e4m3 bytes, scales (optional) s per row.  items: DEVICE array sorted by
 * row0 (prefix sum of rows); one block per row of every item. */
typedef struct {
    const float* src;
    float* dst;
    uint8_t* dst_q;
    float* scales;
    int64_t row0;
    int32_t rows, cols;
} csu_fp8_item;
int csu_quant_e4m3_batch(const csu_fp8_item* items, int count, long total_rows, void* stream);
/* The same quantisation written straight into bf16 shadows: per item (rows x cols fp32, cols % 16 ==
 * 0), scales[row] = s (optional), q (optional) the e4m3 bytes, shadow (rows x cols bf16) = q * s exactly,
 * shadow_t (cols x rows bf16, optional) its transpose; q_perm / q_t / q_tp (optional; rows % 64 == 0 and
 * cols % 64 == 0) the fp8 fused Mlp's byte layouts of q.  items: DEVICE array sorted by blk0 (prefix sum of
 * ceil(rows / 64)); one 256-thread block per 64 rows of every item. */
typedef struct {
    const float* src;
    uint8_t* q;
    float* scales;
    void* shadow;
    void* shadow_t;
    uint8_t* q_perm;   /* optional: e4m3 bytes with columns permuted in 64-groups (dst 32h+16t+4g+i <- src 32t+8g+4h+i) */
    uint8_t* q_t;      /* optional: transposed e4m3 bytes (cols x rows) */
    uint8_t* q_tp;     /* optional: transposed, columns permuted as q_perm (the fp8 fused Mlp's W1^T layout) */
    int64_t blk0;
    int32_t rows, cols;
} csu_fp8_shadow_item;
int csu_quant_e4m3_shadow_batch(const csu_fp8_shadow_item* items, int count, long total_blocks, void* stream);

/* e4m3 byte layouts of quantised weights (the fp8 fused Mlp's operand images): per item, src is a
 * rows x cols byte matrix; mode bit 0 = transpose (dst is cols x rows), bit 1 = permute the dst
 * columns inside every 64-column block: dst column 32h + 16t + 4g + i (h, t in {0,1}, g, i in 0..3)
 * takes column 32t + 8g + 4h + i of the (transposed) source -- the k order in which a 32x32 MFMA
 * accumulator tile pair reaches an f8 operand lane.  Permuting modes need a dst column count
 * % 64 == 0; every mode needs dst columns % 4 == 0.  items: DEVICE array sorted by word0 (prefix sum
 * of the items' dst sizes in 4-byte words); one thread per dst word. */
typedef struct {
    const uint8_t* src;
    uint8_t* dst;
    int64_t word0;
    int32_t rows, cols;        /* of src */
    int32_t mode;
    int32_t pad;
} csu_e4m3_layout_item;
int csu_e4m3_layout_batch(const csu_e4m3_layout_item* items, int count, long total_words, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused multi-tensor AdamW step (torch.optim.AdamW semantics, cswin:937-941): for every item,
 * param *= 1 - lr*wd; m = lerp(m, g, 1-beta1); v = beta2 v + (1-beta2) g^2;
 * param -= lr/(1-beta1^t) * m / (sqrt(v)/sqrt(1-beta2^t) + eps).  items: DEVICE array sorted
 * by chunk0 = first chunk index of the item (chunk0[i+1] = chunk0[i] + the item's chunk count,
 * see below); total_chunks = the sum.  lr_dev / step_dev: device scalars (HIP graph capture) or
 * NULL to use lr / step.  Replaces torch's fused AdamW launches.
 * Optional bf16 shadows of the UPDATED parameter, written in the same pass (the weight copies the
 * next forward's kernels read; they replace the csu_cast_bf16_batch refresh):
 *   shadow == NULL                : no shadow; ceil(numel / csu_adamw_chunk_elems()) chunks.
 *   taps == 0, shadow_t == NULL   : shadow = bf16 param (same layout); ceil(numel / chunk) chunks.
 *   taps == 0, shadow_t != NULL   : the param is a rows x cols matrix processed in 64 x 64 tiles
 *                                   (ceil(rows/64) * ceil(cols/64) chunks): shadow = bf16 W,
 *                                   shadow_t = bf16 W^T (cols x rows).
 *   taps > 0                      : conv weight [rows=N][cols=C][taps=KH*KW]: shadow = OHWI with
 *                                   channel stride cols_pad (>= C), shadow_t = IHWO (or NULL);
 *                                   ceil(numel / chunk) chunks.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    int64_t chunk0;
    void* shadow;
    void* shadow_t;
    int32_t rows, cols;
    int32_t taps, cols_pad;
} csu_adamw_item;
long csu_adamw_chunk_elems(void);
int csu_adamw_step(const csu_adamw_item* items, int count, long total_chunks, const float* lr_dev, float lr,
                   float beta1, float beta2, float eps, float weight_decay, const float* step_dev, float step,
                   void* stream);
/* The same step with torch.optim.Adam's coupled L2 decay (the plain UNet's optimizer,
 * unet:486-490): g += wd * param, no decoupled decay. */
int csu_adam_l2_step(const csu_adamw_item* items, int count, long total_chunks, const float* lr_dev, float lr,
                     float beta1, float beta2, float eps, float weight_decay, const float* step_dev, float step,
                     void* stream);

/* ---------------------------------------------------------------------------------------
 * Global-norm gradient clipping over a csu_adamw_item table (the optimizer's own: same items, same
 * chunk numbering, only `grad`, numel, chunk0 and the tile fields are read), with no host sync.
 * Sums are fp64 from the element on and in a fixed order (no atomics): equal gradients give a
 * bitwise equal norm.
 *
 * csu_grad_sumsq: partial[chunk] = sum g^2 over the in-bounds elements of every chunk
 *   (total_chunks doubles, csu_grad_norm_workspace bytes).  Replaces the per-tensor
 *   torch.linalg.vector_norm / torch._foreach_norm launches of torch.nn.utils.clip_grad_norm_
 *   (get_total_norm).
 * csu_grad_norm_finish: one workgroup sums n partials (of one or several tables laid side by side)
 *   and writes the device scalars
 *     ctl[0] = norm = (float)sqrt(sum)
 *     ctl[1] = coef = min(1, max_norm / (norm + 1e-6))   (exactly 1 when nothing is clipped;
 *              max_norm <= 0 or infinite: 1, norm-only mode; a NaN norm gives NaN as in torch)
 *     ctl[2] = 1 if the sum is finite, else 0
 *     ctl[3] = 0.
 *   Replaces the stack + vector_norm of the per-tensor norms and the clamp(max_norm / (norm + 1e-6))
 *   of clip_grad_norm_ (clip_grads_with_norm_).
 * csu_grad_scale: g *= *coef_dev in place for every item.  Replaces clip_grad_norm_'s
 *   torch._foreach_mul_(grads, clip_coef) (for optimizers other than csu's).
 * csu_adamw_step_ex: csu_adamw_step (l2 == 0) / csu_adam_l2_step (l2 != 0) on g * ctl[1], the product
 *   rounded on its own before anything else uses it: bitwise equal to csu_grad_scale followed by the
 *   plain step, without touching the gradients in memory.  skip_nonfinite != 0 and ctl[2] == 0: the
 *   launch changes nothing (params, moments and shadows keep their values).  Replaces
 *   _foreach_mul_ + the fused AdamW launches, and a GradScaler-style found-inf skip.
 * ------------------------------------------------------------------------------------- */
size_t csu_grad_norm_workspace(long total_chunks);
int csu_grad_sumsq(const csu_adamw_item* items, int count, long total_chunks, double* partial, void* stream);
int csu_grad_norm_finish(const double* partial, long n, float max_norm, float* ctl, void* stream);
int csu_grad_scale(const csu_adamw_item* items, int count, long total_chunks, const float* coef_dev, void* stream);
int csu_adamw_step_ex(const csu_adamw_item* items, int count, long total_chunks, const float* lr_dev, float lr,
                      float beta1, float beta2, float eps, float weight_decay, const float* step_dev, float step,
                      const float* ctl, int skip_nonfinite, int l2, void* stream);

/* ---------------------------------------------------------------------------------------
 * Exponential moving average (EMA) of the weights over a csu_adamw_item table and a parallel DEVICE
 * array `ema` of fp32 pointers, one per item in item order (NULL: no EMA for that item; each EMA
 * tensor has the item's numel, contiguous and 16-B aligned):
 *     ema <- ema + (1 - d) (param - ema),   d = warmup ? min(decay, n / (n + 9)) : decay
 * where n = *ema_updates_dev counts the EMA updates including this one (a device fp32 scalar the
 * caller increments before the launch; may be NULL without warmup).  No atomics, fixed order: bitwise
 * repeatable.  Replaces a Python ModelEma's per-tensor launches / torch._foreach_lerp_.
 *
 * csu_adamw_step_ema: csu_adamw_step_ex with the EMA update of every item done from the updated
 *   parameter while it is in registers (+ 8 B per parameter, no extra launch).  ctl == NULL: no
 *   clipping (csu_adamw_step / csu_adam_l2_step by l2).  A skipped step (skip_nonfinite != 0 and
 *   ctl[2] == 0) leaves the EMA untouched too; the caller then adds ctl[2] instead of 1 to n.
 *   Parameters, moments and shadows are bitwise those of the step without an EMA.
 * csu_ema_update: the stand-alone update in one launch (for optimizers other than csu's); reads only
 *   param, numel, chunk0 and the tile fields of the items.  csu_adamw_step_ema equals the plain step
 *   followed by it bit for bit.
 * csu_ema_swap: param <-> ema for every element in one launch, and every bf16 shadow layout the item
 *   names re-made from the value now in param, exactly as the step writes them: evaluate on the
 *   averaged weights in place, with every captured pointer still valid.  Swapping twice restores
 *   parameters, EMA and shadows bit for bit.  Replaces a second model or two load_state_dict round
 *   trips (each followed by a csu_cast_bf16_batch re-cast).
 * ------------------------------------------------------------------------------------- */
int csu_adamw_step_ema(const csu_adamw_item* items, int count, long total_chunks, const float* lr_dev, float lr,
                       float beta1, float beta2, float eps, float weight_decay, const float* step_dev, float step,
                       const float* ctl, int skip_nonfinite, int l2, float* const* ema, const float* ema_updates_dev,
                       float ema_decay, int ema_warmup, void* stream);
int csu_ema_update(const csu_adamw_item* items, float* const* ema, int count, long total_chunks,
                   const float* ema_updates_dev, float decay, int warmup, void* stream);
int csu_ema_swap(const csu_adamw_item* items, float* const* ema, int count, long total_chunks, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dropout / DropPath (nn.Dropout cswin:190/193/512, timm DropPath cswin:344/367-368) as one
 * elementwise pass where no producing kernel fuses it:
 *   out[i] = res[i] + row_scale[(i / cols) / rows_per_sample] * keep(site, i) / (1 - p) * x[i]
 * over (rows, cols) row-major, cols % 8 == 0; res (fp32) and row_scale (fp32 per sample: 0 or
 * 1/keep_prob of DropPath) may be NULL; p = 0: no mask.  keep(site, i): Philox4x32-7 counter-based
 * bits (csrc/rng.hpp) of the [seed, counter] snapshot `rng` (device uint64 x 2).  The backward of
 * a site is the same call with res = NULL on the incoming gradient.  csu_dropout_mask writes the
 * 0/1 keep mask of elements [0, n) of a site (tests feed it to the CPU oracle).
 * ------------------------------------------------------------------------------------- */
int csu_dropout_apply(long rows, int cols, int xdtype, const void* x, const float* res, int odtype, void* out,
                      const float* row_scale, long rows_per_sample, const uint64_t* rng, unsigned site, float p,
                      void* stream);
int csu_dropout_mask(long n, const uint64_t* rng, unsigned site, float p, uint8_t* out, void* stream);
/* snap[0..1] = state[0..1]; state[1] += 1 (one kernel: the per-forward RNG snapshot, graph-safe) */
int csu_rng_advance(uint64_t* state, uint64_t* snap, void* stream);
/* DropPath per-sample scale (timm drop_path, cswin:344/367-368): out[b] = keep(site, b) / (1 - p)
 * (element b of the site's mask, as csu_dropout_mask) -- the row_scale operand above. */
int csu_droppath_scale(long n, const uint64_t* rng, unsigned site, float p, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * fp32 GEMMs of the fp32 training path (token Linear forward / input / weight gradient, BASELINE
 * config 2), on the fp32 MFMA.  Row-major, C (M, N):
 *   layout 0: C = A (M,K) B(N,K)^T [+ bias (N)] [+ resid (M,N)]   (nn.Linear forward)
 *   layout 1: C = A (M,K) B(K,N)                                    (input gradient dy W)
 *   layout 2: C = A(K,M)^T B(K,N)                                   (weight gradient dy^T x; token
 *             splits reduced in a fixed order through `workspace`, csu_gemm_f32_workspace bytes)
 * Row lengths (K for A in layouts 0/1, M in layout 2, N, K of B in layout 0) multiples of 4.
 * asum (layout 2 only, or NULL): asum[m] = sum_k A[k][m] -- the bias gradient of dW = dy^T x.
 * ------------------------------------------------------------------------------------- */
size_t csu_gemm_f32_workspace(int layout, long M, int N, long K);
int csu_gemm_f32(int layout, long M, int N, long K, const float* A, const float* B, const float* bias,
                 const float* resid, float* C, float* asum, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused Mlp + residual (Mlp cswin:180-196 with the residual add of CSWinBlock cswin:368):
 * fc1 -> GELU -> fc2 with the 4C hidden layer kept on chip.  x (M, C) bf16; w1 (4C, C) and
 * w2 (C, 4C) bf16 nn.Linear weights; b1 (4C), b2 (C) fp32; res / out (M, C) fp32 (may alias).
 * Backward recomputes h = fc1(x) and writes dh = (dy w2) * gelu'(h) (M, 4C), g = gelu(h)
 * (M, 4C) for the weight gradients and dx = dh w1 (M, C), all bf16.  C in {64, 128, 256}.
 * ------------------------------------------------------------------------------------- */
int csu_mlp_supported(int C);
int csu_mlp_fwd(long M, int C, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                const float* res, float* out, void* stream);
int csu_mlp_bwd(long M, int C, const void* x, const void* dy, const void* w1, const float* b1, const void* w2,
                void* dh, void* g, void* dx, void* stream);
/* Dropout inside the fused Mlp (Mlp.drop cswin:190/193, DropPath cswin:368), train mode:
 *   g  = gelu(fc1(x)) * keep(site_hidden, m * 4C + f) / (1 - p)
 *   out = res + row_scale[m / rows_per_sample] * keep(site_out, m * C + c) / (1 - p) * fc2(g)
 * (keep(): rng.hpp's Philox mask of the snapshot rng = [seed, counter]; row_scale NULL = 1).
 * The backward regenerates the hidden mask: dy must already carry the output mask and DropPath
 * scale (csu_dropout_apply on the same site_out / row_scale), g is written dropped (dW2 operand)
 * and dh = (dy w2) * mask * gelu'(h). */
typedef struct {
    const uint64_t* rng;
    uint32_t site_hidden, site_out;
    float p;                   /* 0 <= p < 1 (p = 0: no element masks, row_scale still applies) */
    const float* row_scale;    /* per-sample DropPath scale (0 or 1/keep_prob), or NULL */
    int64_t rows_per_sample;
} csu_mlp_dropout;
int csu_mlp_fwd_dp(long M, int C, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                   const float* res, float* out, const csu_mlp_dropout* d, void* stream);
int csu_mlp_bwd_dp(long M, int C, const void* x, const void* dy, const void* w1, const float* b1, const void* w2,
                   void* dh, void* g, void* dx, const csu_mlp_dropout* d, void* stream);
/* csu_mlp_bwd_dp (no dropout) whose input h (M, C) bf16 is the output of a LayerNorm of x (CSWinBlock
 * norm2, cswin:366-368: x + Mlp(LN(x))), with that LayerNorm's backward in the same launch: the Mlp's
 * input gradient dX = dH W1 is not written; rounded to bf16 exactly as csu_mlp_bwd_dp stores it, it goes
 * through dx (M, C) fp32 = dres + rstd (g - mean(g) - xhat mean(g xhat)), g = dX * gamma, xhat = (x - mean)
 * rstd, its bf16 copy dx_bf16, and the dgamma / dbeta column partials of every 64-token block into part
 * [M / 64][2C] (reduce them with csu_layernorm_param_reduce_batch, nblocks = M / 64).  x fp32 (M, C); dres
 * fp32 (M, C) or NULL; dh and g (M, 4C) bf16 are bitwise csu_mlp_bwd_dp's; rows_per_image as
 * csu_mlp_dropout.rows_per_sample (the hidden-chunk rotation).  Bitwise reproducible; no atomics.
 * C = 128 or 256, M % 64 == 0 (csu_mlp_bwd_ln_supported). */
int csu_mlp_bwd_ln_supported(long M, int C);
int csu_mlp_bwd_ln(long M, int C, const void* h, const void* dy, const void* w1, const float* b1, const void* w2,
                   void* dh, void* g, long rows_per_image, const float* x, const float* gamma, const float* mean,
                   const float* rstd, const float* dres, float* dx, void* dx_bf16, float* part, void* stream);
/* csu_mlp_bwd_dp that also forms the weight and bias gradients, so dh and g are never written
 * (C = 64 only: csu_mlp_bwd_wgrad_supported).  dx is bitwise csu_mlp_bwd_dp's.  Every workgroup of the
 * persistent launch accumulates dW1 = dh^T x, db1 = colsum(dh), dW2 = dy^T g, db2 = colsum(dy) over its
 * token panels, from the same bf16-rounded dh / g values csu_mlp_bwd_dp stores, and writes one fp32
 * partial into slab1 ([dW1 | db1]) and slab2 ([dW2 | db2]) (sizes: csu_mlp_bwd_wgrad_workspace).  The
 * call fills item1 / item2; csu_wslab_reduce_batch over them (any time later on the same stream, with
 * other items) sums the partials in a fixed order into dw1_db1 (4C*C + 4C fp32: dW1 (4C, C) then db1)
 * and dw2_db2 (C*4C + C fp32: dW2 (C, 4C) then db2).  Bitwise reproducible; no atomics. */
int csu_mlp_bwd_wgrad_supported(int C);
int csu_mlp_bwd_wgrad_workspace(long M, int C, size_t* slab1_bytes, size_t* slab2_bytes);
int csu_mlp_bwd_wgrad(long M, int C, const void* x, const void* dy, const void* w1, const float* b1, const void* w2,
                      void* dx, const csu_mlp_dropout* d, float* slab1, float* slab2, csu_wslab_item* item1,
                      csu_wslab_item* item2, float* dw1_db1, float* dw2_db2, void* stream);
/* csu_mlp_fwd_dp that also applies the NEXT CSWinBlock's norm1 LayerNorm (cswin:357) to its output
 * out (M, C) fp32 in the same launch: ln_out (M, C) bf16 = LN(out) * ln_gamma + ln_beta (eps
 * ln_eps), ln_mean / ln_rstd (M) fp32 as csu_layernorm_fwd writes them.  out must not alias res. */
int csu_mlp_fwd_ln(long M, int C, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                   const float* res, float* out, const csu_mlp_dropout* d, const float* ln_gamma, const float* ln_beta,
                   float ln_eps, void* ln_out, float* ln_mean, float* ln_rstd, void* stream);
/* csu_mlp_bwd_dp at C = 128 (any other C: CSU_E_ARG) on the per-panel kernel instead of the deep weight ring
 * that csu_mlp_bwd_dp runs there.  No product path calls it: it exists for the parity tests of the two kernels,
 * and because the compiled C = 128 forward depends on that kernel being built (DESIGN, "Kept, default-off"). */
int csu_mlp_bwd_per_panel(long M, int C, const void* x, const void* dy, const void* w1, const float* b1, const void* w2,
                          void* dh, void* g, void* dx, const csu_mlp_dropout* d, void* stream);
/* fp8-e4m3 fused Mlp forward (BASELINE config 5, "fp8 MFMA weights"; same math and dropout as
 * csu_mlp_fwd_dp) on v_mfma_scale_f32_32x32x64_f8f6f4 with MX block scales:
 *   h   = x_q W1^T + b1, x_q = x quantised per (token, 32 consecutive channels): scale 2^e, e the
 *         smallest integer with amax <= 448 * 2^e, e4m3fn round-to-nearest-even;
 *   g   = gelu(h) (* hidden dropout), g_q = g quantised per (token, 32 consecutive features);
 *   out = res + (g_q W2^T + b2) (* output dropout, DropPath).
 * w1q: (4C, C) e4m3 rows with power-of-two row scales sw1 (4C); w2p: (C, 4C) e4m3 rows (scales sw2,
 * C) with the columns permuted as csu_e4m3_layout_batch mode 2.  C in {64, 128, 256}. */
int csu_mlp_fp8_supported(int C);
int csu_mlp_fp8_fwd(long M, int C, const void* x, const void* w1q, const float* sw1, const float* b1,
                    const void* w2p, const float* sw2, const float* b2, const float* res, float* out,
                    const csu_mlp_dropout* d, void* stream);
/* the same with the NEXT CSWinBlock's norm1 (cswin:357) on its output, as csu_mlp_fwd_ln (bf16 ln_out,
 * fp32 mean / rstd; out must not alias res) */
int csu_mlp_fp8_fwd_ln(long M, int C, const void* x, const void* w1q, const float* sw1, const float* b1,
                       const void* w2p, const float* sw2, const float* b2, const float* res, float* out,
                       const csu_mlp_dropout* d, const float* ln_gamma, const float* ln_beta, float ln_eps, void* ln_out,
                       float* ln_mean, float* ln_rstd, void* stream);
/* Its backward (straight-through for every quantisation): h recomputed exactly as the forward;
 *   dg = (dy * sw2)_q W2q: w2t = W2q^T (4C, C) e4m3 (layout mode 1), dy quantised per (token, 32
 *        consecutive channels) after the per-channel scale sw2 (W2's row scale lies along this sum);
 *   dh = dg * gelu'(h) (* hidden mask) -> dh (bf16, M x 4C); g = g_q of the forward (bf16, exact);
 *   dx = (dh * sw1)_q W1q: w1tp = W1q^T (C, 4C) with permuted columns (layout mode 3), dh * sw1
 *        quantised per (token, 32 consecutive features).  dx bf16 (M, C).  dy carries the output mask. */
int csu_mlp_fp8_bwd(long M, int C, const void* x, const void* dy, const void* w1q, const float* sw1,
                    const float* b1, const void* w2t, const float* sw2, const void* w1tp, void* dh, void* g,
                    void* dx, const csu_mlp_dropout* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Implicit-GEMM NHWC convolution (patch embed cswin:505, Merge_Block.conv cswin:376, CARAFE
 * encoder cswin:397/446, plain-UNet DoubleConv 3x3 unet:182/185 and ConvTranspose2d(k2,s2)
 * unet:211 = the dgrad operator).  x (B,H,W,C), y (B,OH,OW,N) channels-last; weights prepared by
 * the caller: w_ohwi = [N][KH][KW][C], w_ihwo = [C][KH][KW][N] (same dtype as activations).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B, H, W, C;        /* input (of the forward conv) */
    int32_t OH, OW, N;         /* output */
    int32_t KH, KW, stride, pad;
} csu_conv_geom;

/* y = conv(x) + bias (bias fp32 or NULL) */
int csu_conv2d_fwd(const csu_conv_geom* g, int dtype, const void* x, const void* w_ohwi, const float* bias,
                   void* y, void* stream);
/* dx = conv^T(dy) (+ bias, used when this operator is a ConvTranspose2d forward) */
int csu_conv2d_dgrad(const csu_conv_geom* g, int dtype, const void* dy, const void* w_ihwo, const float* bias,
                     void* dx, void* stream);
/* Either operator with an explicit kernel choice (op 0: csu_conv2d_fwd, 1: csu_conv2d_dgrad; src /
 * w as there).  cfg -1: the per-shape choice the plain entries make; 0: the register-staged v2
 * implicit GEMM; 1 + k: the persistent LDS-DMA kernel (bf16, gathered channels % 64 == 0) in tile
 * configuration k (0: 128x128 3-stage, 1: 256x128 2-stage 8 waves, 2: 256x128 3-stage 8 waves,
 * 3: 128x64 4-stage, 4: 256x64 3-stage 8 waves, 5: 128x64 3-stage, 6 / 7: 256x256 8 waves, 8:
 * 512x64 8 waves, 9: 64x64 4-stage, 10: 128x64 3-stage, 11: 64x128 3-stage, the last three two
 * workgroups per CU); 20: the halo kernel of 3x3 stride-1 pad-1 convs with 64 gathered and 64 output
 * channels (H % 2 == 0, W % 64 == 0); 21: the 16 -> 144 channel 3x3 stride-1 pad-1 kernel and its input
 * gradient (W % 64 == 0); CSU_E_ARG when not eligible. */
int csu_conv2d_ex(int op, const csu_conv_geom* g, int dtype, const void* src, const void* w, const float* bias, void* out,
                  int cfg, void* stream);
/* The plain operators with a workspace (op 0: csu_conv2d_fwd, 1: csu_conv2d_dgrad): one-problem bf16
 * convolutions with fewer output tiles than two per CU (the CSWin CARAFE encoders at 16x16 / 32x32)
 * split their K range over workgroups, write fp32 partials into the workspace and sum them in fixed
 * order (+ bias) in a second kernel.  csu_conv2d_workspace: the bytes that split needs (0: no split
 * for this geometry; a NULL or smaller workspace runs unsplit). */
size_t csu_conv2d_workspace(int op, const csu_conv_geom* g, int dtype);
int csu_conv2d_fwd_ws(const csu_conv_geom* g, int dtype, const void* x, const void* w_ohwi, const float* bias, void* y,
                      void* workspace, size_t ws_bytes, void* stream);
int csu_conv2d_dgrad_ws(const csu_conv_geom* g, int dtype, const void* dy, const void* w_ihwo, const float* bias,
                        void* dx, void* workspace, size_t ws_bytes, void* stream);
size_t csu_conv2d_wgrad_workspace(const csu_conv_geom* g);
/* dw_db fp32 [N*KH*KW*C + N] = dW in [N][KH][KW][C] order, then db (sum of dy) */
int csu_conv2d_wgrad(const csu_conv_geom* g, int dtype, const void* x, const void* dy, float* dw_db,
                     void* workspace, size_t ws_bytes, void* stream);
/* the same gradient written in torch's Conv2d weight layout: dw_db fp32 [N*c_real*KH*KW + N] = dW
 * (N, c_real, KH, KW) then db; input channels >= c_real (zero padding of a few-channel input) are
 * dropped.  Same workspace. */
int csu_conv2d_wgrad_oihw(const csu_conv_geom* g, int dtype, const void* x, const void* dy, int c_real, float* dw_db,
                          void* workspace, size_t ws_bytes, void* stream);
/* Weight gradient with an explicit kernel choice: c_real 0 = csu_conv2d_wgrad's [N][KH][KW][C]
 * layout, > 0 = csu_conv2d_wgrad_oihw's.  cfg -1: the per-shape choice of the plain entries; 0: the
 * register-staged v2 kernel; 1 + k: the LDS-DMA kernel (bf16, C % 8 == 0, N % 8 == 0) in tile
 * configuration k (0: 128x128 3-stage, 1: 64x256 3-stage, 2: 128x128 2-stage, 3: 256x128 2-stage 8
 * waves, 4: 64x128 4-stage; 5 / 6: the halo kernel of 3x3 / stride 1 / pad 1 convs with OW % 64 == 0,
 * C % 64 == 0 and N % 64 (5) / N % 128 (6) == 0).  Its workspace: csu_conv2d_wgrad_workspace_ex(g, cfg) (0 when not
 * eligible). */
size_t csu_conv2d_wgrad_workspace_ex(const csu_conv_geom* g, int cfg);
/* Two-source input: the conv of UNet Up over cat([x2, x1], channels) (unet:213-216) without the
 * concatenated tensor.  x holds input channels [0, c_split) (c_split per pixel), x2 channels
 * [c_split, C) (C - c_split per pixel); the input gradient is written the same way (dx / dx2), and
 * the weight gradient reads both (torch OIHW layout + db, csu_conv2d_wgrad_oihw's workspace).
 * csu_conv2d_split_ok: 1 when a geometry / split is supported (bf16 only; 3x3 stride-1 pad-1 with
 * OW % 64 == 0, C, N and c_split multiples of 64); the three calls fail with CSU_E_UNSUPPORTED
 * otherwise (the caller then materialises the concatenation). */
int csu_conv2d_split_ok(const csu_conv_geom* g, int c_split);
int csu_conv2d_fwd_split(const csu_conv_geom* g, int dtype, const void* x, const void* x2, int c_split, const void* w_ohwi,
                         const float* bias, void* y, void* stream);
int csu_conv2d_dgrad_split(const csu_conv_geom* g, int dtype, const void* dy, const void* w_ihwo, void* dx, void* dx2,
                           int c_split, void* stream);
int csu_conv2d_wgrad_split_oihw(const csu_conv_geom* g, int dtype, const void* x, const void* x2, int c_split, const void* dy,
                                float* dw_db, void* workspace, size_t ws_bytes, void* stream);
int csu_conv2d_wgrad_ex(const csu_conv_geom* g, int dtype, const void* x, const void* dy, int c_real, float* dw_db,
                        void* workspace, size_t ws_bytes, int cfg, void* stream);

/* The launch plan of a convolution call: which kernel csu_conv2d_fwd / _dgrad / _wgrad and their
 * _ws / _ex / _split forms run for (op, geometry, dtype, cfg, wgs, c_split, ws_bytes) and how the
 * persistent kernels divide their tiles.  Host only: it touches the device for the CU count alone
 * (256 without a GPU).  It is the function the launches themselves take every decision from, so the
 * report cannot differ from what is launched. */
enum csu_conv_family {
    CSU_CONV_GEMM = 0,        /* conv_gemm: scalar-gather tiles (fp32, or bf16 with channels % 4 != 0) */
    CSU_CONV_IGEMM = 1,       /* igemm_bf16: register-staged v2 implicit GEMM, one tile per workgroup */
    CSU_CONV_IGEMM_DMA = 2,   /* igemm_dma: persistent LDS-DMA implicit GEMM */
    CSU_CONV_HALO64 = 3,      /* conv3_halo64 */
    CSU_CONV_C16 = 4,         /* conv3_c16 */
    CSU_CONV_C16D = 5,        /* conv3_c16d */
    CSU_CONV_WGRAD = 6        /* op 2: the weight-gradient kernel named by wgrad_pick */
};
enum csu_conv_wgrad_v2 {      /* the kernel behind wgrad_pick -1 */
    CSU_WGRAD_V2_NONE = 0,        /* wgrad_pick >= 0 */
    CSU_WGRAD_V2_BF16 = 1,        /* conv_wgrad_bf16<false>: C % 8 == 0, N % 8 == 0, operands below 2 GiB */
    CSU_WGRAD_V2_BF16_N4 = 2,     /* conv_wgrad_bf16<true>: N % 4 == 0 */
    CSU_WGRAD_V2_BF16_WIDE = 3,   /* conv_wgrad_kernel<bf16, vector gathers>: 64-bit offsets or N % 4 != 0 */
    CSU_WGRAD_V2_BF16_SCALAR = 4, /* conv_wgrad_kernel<bf16, scalar gathers>: C % 8 != 0 */
    CSU_WGRAD_V2_F32 = 5,         /* conv_wgrad_kernel<float, vector gathers> */
    CSU_WGRAD_V2_F32_SCALAR = 6   /* conv_wgrad_kernel<float, scalar gathers> */
};
#define CSU_CONV_PLAN_PHASES 16
typedef struct {
    int32_t family;           /* csu_conv_family of the first problem (every problem's: phase_family) */
    int32_t n_problems;       /* problems launched: 1, or the non-empty stride phases of an input gradient;
                               * the per-phase arrays report the first CSU_CONV_PLAN_PHASES of them */
    int32_t two_source;       /* c_split (two sources / two destinations), else 0 */
    int32_t cus;              /* CU count the heuristics used (rounded up to a multiple of 8) */
    int32_t ksplit, kper;     /* K parts of the v2 launch (1: none) and gathered columns per part */
    int32_t v2_bn, v2_vw;     /* IGEMM: output columns per tile (32 narrow / 64) and gather vector width; else 0 */
    int32_t gemm_vec;         /* GEMM: 1 = the 8-channel vector gathers */
    /* the largest and smallest tile (item) count of any workgroup over all problems, and the
     * workgroups that get none */
    int32_t wg_tiles_max, wg_tiles_min, wgs_idle;
    int32_t phase_family[CSU_CONV_PLAN_PHASES];
    int32_t phase_cfg[CSU_CONV_PLAN_PHASES];      /* the csu_conv2d_ex cfg that forces this choice: 0 v2, 1 + k, 20,
                                                   * 21; -1 for GEMM */
    int32_t phase_bm[CSU_CONV_PLAN_PHASES];       /* tile rows and columns (HALO64: 128 x 64, C16 / C16D: 64 x N) */
    int32_t phase_bn[CSU_CONV_PLAN_PHASES];
    int32_t phase_ring[CSU_CONV_PLAN_PHASES];     /* ring stages S of the persistent kernels, else 0 */
    int64_t phase_rows[CSU_CONV_PLAN_PHASES];     /* GEMM rows M */
    int64_t phase_tiles[CSU_CONV_PLAN_PHASES];    /* tiles or items */
    int32_t phase_nk[CSU_CONV_PLAN_PHASES];       /* K slices per tile (HALO64 / C16 / C16D: 1) */
    int32_t phase_grid[CSU_CONV_PLAN_PHASES];     /* workgroups launched for the problem */
    int32_t phase_tiles_max[CSU_CONV_PLAN_PHASES];
    int32_t phase_tiles_min[CSU_CONV_PLAN_PHASES];
    int32_t phase_idle[CSU_CONV_PLAN_PHASES];
    int32_t phase_xcd_rem[CSU_CONV_PLAN_PHASES];  /* tiles % 8 of the persistent kernels, else 0 */
    /* op 2 */
    int32_t wgrad_pick;       /* -1 the v2 kernels, else the configuration k of csu_conv2d_wgrad_ex's cfg 1 + k */
    int32_t wgrad_chunks;     /* row (halo: segment) chunks, one partial slab each */
    int32_t wgrad_v2;         /* csu_conv_wgrad_v2 */
    int32_t _pad;
    int64_t wgrad_rpc;        /* rows (halo: 64-pixel segments) per chunk */
    int64_t wgrad_last;       /* rows (segments) of the last chunk */
    uint64_t wgrad_ws_bytes;  /* workspace the call needs */
} csu_conv_plan;
/* op 0 forward, 1 input gradient, 2 weight gradient.  cfg as csu_conv2d_ex (op 0 / 1) or
 * csu_conv2d_wgrad_ex (op 2).  wgs: 0, or the persistent grid (csu_conv2d_ex2).  c_split: 0, or the
 * two-source split.  ws_bytes: workspace of a _ws call (0: none).  Runs the same validation as the
 * launches; 0 or a csu_status. */
int csu_conv2d_plan(int op, const csu_conv_geom* g, int dtype, int cfg, int wgs, int c_split, size_t ws_bytes,
                    csu_conv_plan* out);
/* csu_conv2d_ex with every choice explicit (tests, tuning).  second / c_split: NULL / 0, or the
 * two-source form (op 0: second = x2, op 1: second = dx2; needs csu_conv2d_split_ok).  wgs: 0 = the
 * grid the plain entries launch (1 or 2 workgroups per CU); otherwise the number of persistent
 * workgroups of igemm_dma, conv3_halo64, conv3_c16 and conv3_c16d, a positive multiple of 8 (the
 * kernels give each of the 8 XCDs gridDim.x / 8 workgroups) of at most 65536, else CSU_E_ARG; the
 * one-tile-per-workgroup kernels ignore it.  workspace / ws_bytes as the _ws entries (NULL / 0: none). */
int csu_conv2d_ex2(int op, const csu_conv_geom* g, int dtype, const void* src, const void* w, const float* bias, void* out,
                   void* second, int c_split, int cfg, int wgs, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Step glue (csrc/glue.hip), the elementwise passes between the kernels above:
 * grad_join: out (fp32, n) = a + b (b may be NULL), plus out_bf16 (bf16 copy, or NULL); a / b
 *   bf16 or fp32, n % 8 == 0; out NULL with out_bf16 set: a bf16 cast of a (+ b).  The gradient of an fp32 activation cast once to bf16 for two
 *   consumers (encoder skip cswin:530-545/568-592, CARAFE input cswin:408-432).
 * bce_loss: nn.BCELoss(reduction='mean') (cswin:935) on probabilities p and targets t (fp32, n):
 *   loss[0] = mean(-(t max(log p, -100) + (1-t) max(log(1-p), -100))), deterministic; backward
 *   dp = dloss[0] (p - t) / max((1-p) p, 1e-12) / n.
 * pack_nhwc_bf16: fp32 NCHW image (B, C, H, W) -> bf16 NHWC (B, H, W, Cp), channels >= C zero
 *   (the patch-embed conv input, cswin:505).
 * ------------------------------------------------------------------------------------- */
int csu_grad_join(long n, int adtype, const void* a, int bdtype, const void* b, float* out, void* out_bf16,
                  void* stream);
size_t csu_bce_loss_workspace(long n);
int csu_bce_loss_fwd(long n, const float* p, const float* t, float* loss, void* workspace, size_t ws_bytes,
                     void* stream);
/* the same loss plus the reference loop's per-step segmentation sums (cswin:789-795, pred = p > 0.5):
 * stats[0] = sum(pred * t), stats[1] = sum(pred), stats[2] = sum(t) (fp32, fixed order) */
int csu_bce_loss_fwd_stats(long n, const float* p, const float* t, float* loss, float* stats, void* workspace,
                           size_t ws_bytes, void* stream);
int csu_bce_loss_bwd(long n, const float* p, const float* t, const float* dloss, float* dp, void* stream);
int csu_pack_nhwc_bf16(int B, int C, int H, int W, int Cp, const float* x, void* y, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused segmentation loss (csrc/seg_loss.hip): BCE + Tversky (Dice is alpha = beta = 0.5) on fp32
 * probabilities p and targets t (n elements) viewed as rows x (n / rows); rows = 1 is the
 * batch-flattened form of the Dice metric (cswin:692-698), rows = B the per-image form.  Per row r:
 *   TP = sum p t, P = sum p, T = sum t, D = (1 - alpha - beta) TP + alpha P + beta T + smooth,
 *   TI = (TP + smooth) / D;
 *   BCE = (1/n) sum -(pos_weight t max(log p, -100) + (1 - t) max(log1p(-p), -100));
 *   loss[0] = w_bce BCE + w_tversky mean_r(1 - TI_r), deterministic (fixed-order sums, no atomics).
 * fwd also writes coef (rows x 2 floats: A_r = (D - (TP + smooth)(1 - alpha - beta)) / D^2,
 * C_r = alpha (TP + smooth) / D^2) for bwd and, with stats != NULL, the thresholded sums of
 * csu_bce_loss_fwd_stats over the whole batch (stats[0] = sum(pred * t), stats[1] = sum(pred),
 * stats[2] = sum(t), pred = p > 0.5).  Workspace csu_seg_loss_workspace(n, rows) bytes.
 * bwd: dp = dloss[0] (w_bce (p (1 - t) - pos_weight t (1 - p)) / max(p (1 - p), 1e-12) / n
 *                     - (w_tversky / rows) (t A_r - C_r));  at pos_weight 1 the first term is bce_loss's.
 * CSU_E_ARG: n < 1, rows < 1, n % rows != 0, smooth <= 0, a negative weight, alpha, beta or
 * pos_weight, or both weights zero.  Any address alignment is accepted (16-B accesses are used
 * where p, t and dp share their offset within 16 B).
 * ------------------------------------------------------------------------------------- */
size_t csu_seg_loss_workspace(long n, int rows);
int csu_seg_loss_fwd(long n, int rows, const float* p, const float* t, float w_bce, float pos_weight, float w_tversky,
                     float alpha, float beta, float smooth, float* loss, float* stats, float* coef, void* workspace,
                     size_t ws_bytes, void* stream);
int csu_seg_loss_bwd(long n, int rows, const float* p, const float* t, const float* dloss, const float* coef,
                     float w_bce, float pos_weight, float w_tversky, float* dp, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused multi-class segmentation loss (csrc/seg_ce.hip): softmax cross-entropy + per-class
 * Tversky (Dice is alpha = beta = 0.5) on K-class logits and integer labels.  The reference has no
 * counterpart: it trains num_classes=1 with nn.BCELoss (cswin:924, 936).
 *   z: logits of B images x K classes x HW pixels, dtype CSU_F32 or CSU_BF16 (upcast in registers),
 *      element (b, k, pix) at z[b s_b + k s_k + pix s_pix]; class-last (s_k = 1, s_pix = pitch >= K)
 *      and NCHW (s_pix = 1) are read with vector loads, anything else per element.  pad_ok != 0:
 *      with s_k = 1 and s_pix >= KB (K rounded up to 4, 8, 16 or 32) the KB elements from every
 *      pixel's start lie inside the allocation (a [..., :K] view of a padded GEMM output) and may be
 *      read (dz: written, as zeros).
 *   t: labels, B x HW contiguous, label_dtype 0 = uint8, 1 = int64.  A pixel with t == ignore_index
 *      contributes to no sum and gets a zero gradient; other labels outside [0, K) are a caller
 *      error (they match no class; no label indexes memory).
 *   p = softmax_k(z) in fp32; rows = 1 (one Tversky row for the batch) or B (one per image):
 *   CE = sum_pix w[t] (logsumexp(z) - z_t) / sum_pix w[t]   (w = class_weight, NULL: 1); 0, with a
 *        zero gradient, when every pixel is ignored (F.cross_entropy gives NaN there);
 *   TP_rc = sum p_c [t = c], P_rc = sum p_c, T_rc = sum [t = c], D = (1 - alpha - beta) TP + alpha P + beta T + smooth,
 *   loss[0] = w_ce CE + w_tversky mean_r mean_{c in C} (1 - (TP + smooth) / D),  C = all classes, or
 *        1 .. K-1 with include_background = 0.  Deterministic (fixed-order sums, no atomics).
 * fwd also writes coef (csu_seg_ce_coef_floats = 2 rows K + 1 floats: per (row, class) A = (D - (TP +
 * smooth)(1 - alpha - beta)) / D^2 and C = alpha (TP + smooth) / D^2, zero for an excluded background;
 * then 1 / sum w) and, with stats != NULL, the fp64 (3, K) hard sums over the batch of pred =
 * argmax_k z (lowest index wins a tie): stats[c] = sum [pred = c][t = c], stats[K + c] = sum [pred = c],
 * stats[2 K + c] = sum [t = c].  Workspace csu_seg_ce_workspace(B, K, HW) bytes (0: bad arguments).
 * bwd: dz_k = dloss[0] (w_ce w[t] (p_k - [k = t]) / sum w
 *                      - (w_tversky / (rows |C|)) p_k (G_k - sum_c G_c p_c)),  G_c = A_rc [t = c] - C_rc,
 * written in the logits' dtype with the logits' strides.
 * CSU_E_ARG: B or HW < 1, K < 2 or K > 32, rows not 1 or B, a dtype other than the above, a stride
 * < 1, smooth <= 0, a negative weight, alpha or beta, both weights zero, a null pointer.
 * ------------------------------------------------------------------------------------- */
size_t csu_seg_ce_workspace(int B, int K, long HW);
int csu_seg_ce_fwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix, int pad_ok,
                   int label_dtype, const void* t, long ignore_index, const float* class_weight, float w_ce,
                   float w_tversky, float alpha, float beta, float smooth, int include_background, float* loss,
                   double* stats, float* coef, void* workspace, size_t ws_bytes, void* stream);
int csu_seg_ce_bwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix, int pad_ok,
                   int label_dtype, const void* t, long ignore_index, const float* class_weight, const float* dloss,
                   const float* coef, float w_ce, float w_tversky, int include_background, void* dz, void* stream);

/* ---------------------------------------------------------------------------------------
 * The same loss with a boundary term (Kervadec et al. 2019, "Boundary loss for highly unbalanced
 * segmentation"; csrc/seg_ce.hip, the kernels above with one compile-time flag set); the reference has
 * no counterpart.  Every argument of csu_seg_ce_* keeps its meaning; added:
 *   phi:  dense fp32 (B, K, HW), phi[b, c, pix] = the signed distance of the pixel to the border of class c
 *         in the label map (csu_signed_distance: negative inside the class); read as data, must be finite.
 *   w_bd: one float on the device, read by the kernels, so a schedule can change the weight between
 *         replays of a captured graph.  It is not checked.
 *   bd_background: 0 = the classes 1 .. K-1 carry the term, 1 = all K classes; that set is Cb.
 *   n  = sum_c T_c                                     (the live pixels whose label is a class, whole batch)
 *   BD = (1 / (n |Cb|)) sum over live pixels, c in Cb of p_c phi_c               (0 when n = 0)
 *   loss[0] = [w_ce CE + w_tversky ...] + w_bd[0] BD;  terms[0] = the bracket, terms[1] = BD
 *   dz_k   += dloss[0] w_bd[0] / (n |Cb|) p_k (f_k - sum_c f_c p_c),   f_c = phi_c for c in Cb, else 0
 * fwd keeps one more partial sum per (image, chunk) item, in the same fixed order, divides in fp64 and
 * leaves 1 / (n |Cb|) behind 1 / sum w in coef (2 rows K + 2 floats).  Workspace csu_seg_bd_workspace(B, K,
 * HW) bytes = (3 + 5 K) floats per item (0: bad arguments).  w_ce = w_tversky = 0 is legal here.
 * Ignored pixels contribute nothing and get a zero gradient; deterministic, no atomics.  With w_bd[0] = 0
 * the loss and dz equal those of csu_seg_ce_* on the same inputs.
 * CSU_E_ARG: as csu_seg_ce_* (but for the two zero weights), a null phi, w_bd or terms.
 * ------------------------------------------------------------------------------------- */
size_t csu_seg_bd_workspace(int B, int K, long HW);
int csu_seg_bd_fwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix, int pad_ok,
                   int label_dtype, const void* t, long ignore_index, const float* class_weight, float w_ce,
                   float w_tversky, float alpha, float beta, float smooth, int include_background, const float* phi,
                   const float* w_bd, int bd_background, float* loss, float* terms, double* stats, float* coef,
                   void* workspace, size_t ws_bytes, void* stream);
int csu_seg_bd_bwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix, int pad_ok,
                   int label_dtype, const void* t, long ignore_index, const float* class_weight, const float* dloss,
                   const float* coef, float w_ce, float w_tversky, int include_background, const float* phi,
                   const float* w_bd, int bd_background, void* dz, void* stream);

/* ---------------------------------------------------------------------------------------
 * The k-th largest of cap fp32 keys, k a fraction of the live ones (csrc/kth_largest.hip): the threshold of
 * the top-k cross-entropy below; the reference has no counterpart.
 *   keys: cap floats on the device; a key with the sign bit set is skipped.  The others are compared by their
 *         bit patterns, which order +0, denormals, normals and +inf as their values do (a NaN sorts above +inf).
 *   rho:  one float on the device.  n = the keys not skipped, k = max(1, floor((double)rho[0] n)), at most n.
 *   out:  5 doubles on the device: tau = the k-th largest key (exactly the float), n_gt = #{key > tau},
 *         n_eq = #{key = tau}, k, n.  n = 0: all zero.
 * A 4 x 8-bit radix select with integer histograms: exact, the same for any order of the keys, nothing returns
 * to the host, and no loop bound is read from device memory.  Workspace csu_kth_largest_workspace(cap) bytes,
 * 8-byte aligned (0: cap < 1).
 * CSU_E_ARG: cap < 1 or > 2^40, a null or misaligned pointer.
 * ------------------------------------------------------------------------------------- */
size_t csu_kth_largest_workspace(long cap);
int csu_kth_largest(long cap, const float* keys, const float* rho, double* out, void* workspace, size_t ws_bytes,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * The multi-class loss with a hard-example CE term: focal weighting (Lin et al. 2017) and / or a top-k
 * selection over the batch (nnU-Net's TopKLoss); csrc/seg_ce.hip, the kernels above with one more
 * compile-time flag.  The reference has no counterpart.  Every argument of csu_seg_ce_* keeps its meaning; added:
 *   gamma: >= 0, finite.   rho: one float on the device, or NULL for no selection.
 *   keys:  B HW floats, written by fwd and read by bwd; NULL exactly when rho is.
 * For a live pixel (label in [0, K), not ignore_index), p = softmax(z), q = p_t:
 *   u = sum_{k != t} p_k,  L = logsumexp(z) - z_t,  l = w[t] u^gamma L   (u^gamma = 1 at gamma = 0; l >= +0)
 *   no rho: HCE = sum l / sum w[t]                                                    (0 when sum w[t] = 0)
 *   rho:    (tau, n_gt, n_eq, k, n) = csu_kth_largest of the l (keys[pix] = l, a dead pixel: -1), f = (k - n_gt) / n_eq,
 *           m = 1 (l > tau), f (l = tau), 0 (l < tau),  HCE = sum m l / sum m w[t]   (0 when the denominator W is 0)
 *   loss[0] = w_ce HCE + w_tversky mean_r mean_{c in C} (1 - TI_rc);  terms = fp64 {HCE, the Tversky mean, tau, k}
 *             (no rho: tau = 0, k = the live pixels)
 *   dz_k = dloss[0] (w_ce m w[t] (p_k - [k = t]) (u^gamma + gamma q u^(gamma - 1) L) / W - the Tversky part of csu_seg_ce_bwd);
 *          the second summand is 0 at gamma = 0, u = 0 or L = 0.  m is taken from keys and tau, never from an l
 *          formed again.
 * coef: 2 rows K + 3 floats (A, C per (row, class), then 1 / W, tau, f).  Workspace csu_seg_hard_workspace(B, K, HW)
 * bytes (a multiple of 8), 8-byte aligned: csu_kth_largest's, 6 doubles, and (5 + 5 K) floats per (image, chunk) item.
 * Deterministic: fixed-order sums and integer atomics only.
 * CSU_E_ARG: as csu_seg_ce_*, gamma negative or not finite, rho without keys or keys without rho, a null terms.
 * ------------------------------------------------------------------------------------- */
size_t csu_seg_hard_workspace(int B, int K, long HW);
int csu_seg_hard_fwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix, int pad_ok,
                     int label_dtype, const void* t, long ignore_index, const float* class_weight, float w_ce,
                     float w_tversky, float alpha, float beta, float smooth, int include_background, float gamma,
                     const float* rho, float* keys, float* loss, double* terms, double* stats, float* coef,
                     void* workspace, size_t ws_bytes, void* stream);
int csu_seg_hard_bwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix, int pad_ok,
                     int label_dtype, const void* t, long ignore_index, const float* class_weight, const float* dloss,
                     const float* coef, float w_ce, float w_tversky, int include_background, float gamma,
                     const float* keys, void* dz, void* stream);

/* ---------------------------------------------------------------------------------------
 * Stable segmented radix sort of (uint32 key, uint32 value) pairs (csrc/sort_pairs.hip): the order of the
 * Lovasz-Softmax loss below; the reference has no counterpart.
 *   keys, vals: segments x len pairs on the device, `segments` contiguous runs of `len` pairs.  Each run is
 *               sorted on its own, ascending by the low key_bits (1 .. 32) bits of the key; the bits above
 *               are carried along and ignored.  Pairs with equal keys keep their order (stable).  The
 *               result lands in keys / vals; keys_alt / vals_alt (the same size) are scratch.
 * An LSD sort by 8-bit digits, ceil(key_bits / 8) passes of three launches: a digit histogram per tile of
 * csu_sort_pairs_tile() pairs, a scan of every digit's row of tile counts, and a scatter that ranks a
 * tile's pairs with wave ballots in their order.  Integers only, no atomics on global memory, nothing to
 * clear: bitwise repeatable and a function of the input alone.  Nothing returns to the host, and no loop
 * bound is read from device memory.  Workspace csu_sort_pairs_workspace(segments, len) bytes, 4-byte
 * aligned (0: bad arguments).
 * CSU_E_ARG: segments < 1, len < 1, segments * len >= 2^31, key_bits outside 1 .. 32, a null or misaligned
 * pointer.  CSU_E_WORKSPACE: a null or short workspace.
 * ------------------------------------------------------------------------------------- */
size_t csu_sort_pairs_workspace(int segments, long len);
int csu_sort_pairs(int segments, long len, int key_bits, uint32_t* keys, uint32_t* vals, uint32_t* keys_alt,
                   uint32_t* vals_alt, void* workspace, size_t ws_bytes, void* stream);
int csu_sort_pairs_tile(void);

/* ---------------------------------------------------------------------------------------
 * The multi-class loss with the Lovasz-Softmax term (Berman, Triki, Blaschko, CVPR 2018), the convex
 * surrogate of the mean IoU; csrc/seg_ce.hip, the kernels above with one more compile-time flag, and
 * csu_sort_pairs.  The reference has no counterpart.  Every argument of csu_seg_ce_* keeps its meaning; added:
 *   class_mask:   bit c set = class c carries the term (the set C, |C| >= 1, no bit at or above K).
 *   present_only: 1 = only the segments with a foreground pixel count (Berman's "present"), 0 = all of C.
 *   per_image:    0 = a segment is one class over the whole batch, 1 = one (image, class) pair.
 *   w_lv:         one float on the device, read by the kernels, so a schedule can change the weight between
 *                 replays of a captured graph.  It is not checked.
 *   sorted_keys, sorted_vals: uint32 (|C|, B, HW), written by fwd: per segment in sorted order
 *                 key = (dead ? 1 << 30 : 0) | (0x3F800000 - bits(e)), value = (fg << 31) | flat index in the
 *                 segment (b HW + pix, or pix with per_image).  A dead pixel (label = ignore_index) has e = 0.
 *   psi:          fp32 (|C|, B, HW), fully written by fwd and read by bwd: dLS / dp_c of every pixel.
 * For a segment of class c with n live pixels in ascending flat index, p = softmax(z):
 *   fg_i = [t_i = c],  e_i = fminf(fg_i ? sum_{k != c} p_k : p_c, 1),  pi = descending e, ties in ascending index
 *   G = sum fg;  for j = 1 .. n:  F = #fg among pi(1 .. j-1),  I = G - F,  U = I + (j - 1),
 *   g_j = 1 / U (pi(j) foreground),  I / (U (U + 1)) (background),  1 (U = 0);   LS_seg = sum_j e_pi(j) g_j
 *   LS = sum over the counted segments of LS_seg / (max(1, number counted) x (B if per_image else 1)), counted
 *        within an image with per_image;   psi = -/+ g_rank scale (foreground / background), 0 for a dead pixel
 *   loss[0] = [w_ce CE + w_tversky ...] + w_lv[0] LS;  terms[0] = the bracket, terms[1] = LS
 *   dz_k   += dloss[0] w_lv[0] p_k (f_k - sum_c f_c p_c),   f_c = psi_c for c in C, else 0
 * fwd: the csu_seg_ce forward with the keys and values written in the same pass, csu_sort_pairs on 31 key
 * bits, a three-launch integer scan of the fg bits over the sorted order, a pass that forms g and psi in fp64
 * from the integers and sums e g per tile in fp64, and a fixed-order finish.  coef: 2 rows K + 2 floats.
 * Workspace csu_seg_lovasz_workspace(B, K, HW, class_mask, per_image) bytes (a multiple of 8), 8-byte aligned
 * (0: bad arguments).  w_ce = w_tversky = 0 is legal here.  Deterministic: fixed-order sums only.  With
 * w_lv[0] = 0 the loss and dz equal those of csu_seg_ce_* on the same inputs bit for bit.
 * CSU_E_ARG: as csu_seg_ce_* (but for the two zero weights), an empty class_mask or one with a bit at or above
 * K, |C| B HW >= 2^31, a null w_lv, sorted_keys, sorted_vals, psi or terms.
 * ------------------------------------------------------------------------------------- */
size_t csu_seg_lovasz_workspace(int B, int K, long HW, uint32_t class_mask, int per_image);
int csu_seg_lovasz_fwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                       int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                       float w_ce, float w_tversky, float alpha, float beta, float smooth, int include_background,
                       uint32_t class_mask, int present_only, int per_image, const float* w_lv, uint32_t* sorted_keys,
                       uint32_t* sorted_vals, float* psi, float* loss, float* terms, double* stats, float* coef,
                       void* workspace, size_t ws_bytes, void* stream);
int csu_seg_lovasz_bwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                       int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                       const float* dloss, const float* coef, float w_ce, float w_tversky, int include_background,
                       uint32_t class_mask, const float* psi, const float* w_lv, void* dz, void* stream);

/* ---------------------------------------------------------------------------------------
 * Mask-aligned batch augmentation (AugmentationTransform cswin:20-87 + the dataset's /255 and
 * HWC -> CHW, cswin:166-173), square S x S images: img uint8 (B, S, S, 3), mask uint8 (B, S, S),
 * params int32 (B, 7) on the device = {hflip, vflip, clockwise quarter turns 0..3, crop top,
 * crop left, crop height, crop width} (the crop taken from the flipped/rotated image and resized
 * back to S x S bilinearly, half-pixel centres, results rounded to uint8 like the reference's
 * uint8 resize); out_img fp32 (B, 3, S, S) = value / 255, out_mask fp32 (B, 1, S, S).
 * ------------------------------------------------------------------------------------- */
int csu_augment_batch(int B, int S, const void* img, const void* mask, const int* params, float* out_img,
                      float* out_mask, void* stream);

/* ---------------------------------------------------------------------------------------
 * Affine + elastic + intensity augmentation with device-drawn parameters (csrc/augment_warp.hip).
 * The reference has no counterpart (its augmentation is csu_augment_batch above); this is the
 * TransUNet / nnU-Net style set, for images, binary masks and label maps, H x W independent.
 *
 * The per-image parameter table is float table[B][CSU_AUGMENT_P]:
 *   [0] hflip (0/1)   [1] vflip (0/1)   [2] clockwise quarter turns k (0..3)
 *   [3] angle (rad, positive turns the content clockwise on screen: x right, y down)
 *   [4] scale   [5] tx   [6] ty (pixels)
 *   [7] contrast   [8] brightness   [9] gamma   [10] noise sigma   [11] elastic magnitude (pixels)
 *   [12..17] A = {a00, a01, a02, a10, a11, a12}: the folded INVERSE affine; the source position of the
 *            output pixel centre (x, y) is (a00 x + a01 y + a02, a10 x + a11 y + a12) in pixel-centre
 *            coordinates.  The content transform is T(t) C R(angle) S(scale) Q(k) F(h, v) C^-1 about
 *            c = ((W - 1) / 2, (H - 1) / 2), so A = C F Q(k)^T R(angle)^T / scale C^-1 T(-t); composed in
 *            fp64 and rounded once: exact for angle = 0, scale = 1 and integer t.
 *   [18..19] reserved (0).
 * The identity values are 0 (flips, k, angle, t, sigma, magnitude) and 1 (scale, contrast, brightness,
 * gamma); the kernels read only [7..17] and skip an intensity step whose parameter is its identity.
 *
 * csu_augment_draw fills the table, and ctrl when it is not NULL, from the [seed, counter] snapshot
 * `rng` (device uint64 x 2, csu_rng_advance): row b is a pure function of (seed, counter, site, b),
 * H, W and cfg -- not of B or the launch shape.  Philox4x32-7 (csrc/rng.hpp), counter words
 * {j, (b << 12) ^ site, counter}; uniforms are (bits >> 8) / 2^24.  Each transform is applied when its
 * uniform is below its probability and keeps its identity value otherwise; a quarter turn that is
 * applied is 1, 2 or 3; scale is log-uniform, everything else uniform in [lo, hi]; tx in
 * [-translate_x, translate_x].  ctrl: float [B][2][Gy][Gx] (x displacements, then y), Gx =
 * ceil(W / spacing) + 3, Gy = ceil(H / spacing) + 3, uniform in [-1, 1) * table[b][11], drawn under
 * site_ctrl.  Limits of the three calls: B <= 2^20 (csu_augment_mean: 65535), H W < 2^31, H <= 262140, sites
 * below 4096, spacing >= 4 when ctrl is given.
 *
 * csu_augment_mean: mean[b] = the mean of image b's n bytes / 255 from an exact 64-bit integer sum
 * (`sums`, B uint64 of scratch, zeroed by the call), so it does not depend on the order of the adds.
 *
 * csu_augment_warp: one pass over the output pixels.  img uint8 (B, H, W, 3), mask uint8 (B, H, W).
 *   position: (x, y) is displaced by the uniform cubic B-spline of ctrl (NULL or magnitude 0: none):
 *     i = x / spacing, f = (x mod spacing) / spacing, d = c00 + sum_ab B_a(f_y) B_b(f_x) (c_ab - c00)
 *     over the 4 x 4 control points from (i_y, i_x) (relative to the first one, so that a constant field
 *     is reproduced exactly), then mapped through A.
 *   border CSU_AUG_CONSTANT: image taps outside read image_fill (in output units, [0, 1]), bilinear mask
 *     taps outside read 0, a nearest mask value outside is pad_label.  CSU_AUG_REPLICATE: the source
 *     coordinate is clamped to the image for all three.
 *   image: bilinear sample, then per channel v = s / 255; v = (v - mean) contrast + mean; v *= brightness;
 *     clamp to [0, 1]; v = v^gamma; v += sigma n; clamp.  n is a standard normal (Box-Muller) of the Philox
 *     call {y W + x, (b << 12) ^ noise_site, counter}: channels 0 / 1 take the cosine / sine branch of its
 *     first pair of words, channel 2 the cosine branch of the second.  rng NULL: no noise.
 *     out_img fp32 (B, 3, H, W).
 *   mask_mode CSU_AUG_MASK_BILINEAR: out_mask fp32 (B, 1, H, W) = bilinear sample / 255, not rounded.
 *     CSU_AUG_MASK_NEAREST: the value at (floor(sx + 0.5), floor(sy + 0.5)) / 255 as fp32 (B, 1, H, W).
 *     CSU_AUG_MASK_LABELS: that value as int64 (B, H, W) (pad_label may be an ignore index such as 255).
 * ------------------------------------------------------------------------------------- */
#define CSU_AUGMENT_P 20
enum csu_augment_border { CSU_AUG_CONSTANT = 0, CSU_AUG_REPLICATE = 1 };
enum csu_augment_mask_mode { CSU_AUG_MASK_BILINEAR = 0, CSU_AUG_MASK_NEAREST = 1, CSU_AUG_MASK_LABELS = 2 };
typedef struct {
    float p_hflip, p_vflip, p_rot90;
    float p_rotate, rotate_lo, rotate_hi;          /* radians */
    float p_scale, scale_lo, scale_hi;             /* > 0 */
    float p_translate, translate_x, translate_y;   /* largest |shift| in pixels */
    float p_contrast, contrast_lo, contrast_hi;
    float p_brightness, brightness_lo, brightness_hi;
    float p_gamma, gamma_lo, gamma_hi;             /* > 0 */
    float p_noise, noise_lo, noise_hi;             /* sigma, >= 0 */
    float p_elastic, elastic_lo, elastic_hi;       /* magnitude in pixels, >= 0 */
    int32_t spacing;                               /* control-grid spacing in pixels (ctrl != NULL) */
} csu_augment_config;
int csu_augment_draw(const csu_augment_config* cfg, int B, int H, int W, const uint64_t* rng, unsigned site,
                     unsigned site_ctrl, float* table, float* ctrl, void* stream);
int csu_augment_mean(int B, long n, const void* img, uint64_t* sums, float* mean, void* stream);
int csu_augment_warp(int B, int H, int W, const void* img, const void* mask, const float* table, const float* ctrl,
                     int spacing, const float* mean, const uint64_t* rng, unsigned noise_site, int border,
                     float image_fill, int pad_label, int mask_mode, float* out_img, void* out_mask, void* stream);

/* ---------------------------------------------------------------------------------------
 * Patch pool: training patches cut on the device from full-size cases kept in HBM (csrc/patch.hip, the warp
 * in csrc/augment_warp.hip).  The reference has no counterpart; this is nnU-Net's patch sampling with forced
 * foreground centres.
 *
 * The pool of N cases (N <= 2^20, each H_i, W_i <= 2^24 and H_i W_i < 2^31):
 *   pixels  uint8, the images HWC (3 bytes per pixel), cases back to back
 *   labels  uint8, one byte per pixel, the same order
 *   meta    int64 [N][4] = {pixel offset (image i starts at pixels + 3 offset and labels + offset), H_i, W_i,
 *           row-table offset (in int32 entries into rows)}
 *   mean    float [N]: csu_augment_mean of each image, the mean the contrast step of a patch of it uses
 *   rows    int32: for image i, class c in 0..Kc-1 and y in 0..H_i,
 *           rows[meta[i][3] + c (H_i + 1) + y] = the number of pixels of class c in rows [0, y) of image i (an
 *           exclusive prefix over rows: the entry at H_i is the class's pixel count); Kc (H_i + 1) entries per image.
 * Classes: K = 1 is the binary case, Kc = 2, class = (label > 0).  Otherwise 2 <= K <= 32, Kc = K, class = label,
 * and a label >= K (an ignore value) belongs to no class.
 *
 * csu_patch_index fills rows (integers only: deterministic).  max_h, the largest H_i, only sizes the launch.
 *
 * csu_patch_draw: record[b], int32 [B][CSU_PATCH_RECORD] = {n, cls, cy, cx, oy, ox, fg, count, w0..w7}, a pure
 * function of (seed, counter, site, b), the pool and the arguments -- not of B.  w0..w3 / w4..w7 are the words of
 * the Philox4x32-7 calls j = 0 / 1 with counter words {j, (b << 12) ^ site, counter} (the scheme of
 * csu_augment_draw), stored as their bit patterns.  pick(w, m) = (uint64(w) m) >> 32; u01(w) = (w >> 8) / 2^24.
 *   image   n = indices[b] clamped to 0..N-1 when indices is not NULL, else pick(w0, N)
 *   foreground iff b < fg_slots or u01(w1) < p_fg
 *   class   of the classes c < Kc with bit c of class_mask set and a nonzero count in image n, m of them in
 *           ascending order, the pick(w2, m)-th; m = 0: the slot becomes a uniform one
 *   pixel   count = that class's pixels in image n, r = pick(w3, count), (cy, cx) = the r-th pixel of the class
 *           in raster order
 *   origin  per axis (L the image's extent, P the patch's, c the centre): L < P: -((P - L) / 2) (centred, the rest
 *           is padding); else foreground: min(max(c - P / 2, 0), L - P); uniform: pick(w4, H - Ph + 1) for oy,
 *           pick(w5, W - Pw + 1) for ox.  Integer divisions of non-negative values.
 *   A uniform slot (not foreground, or no eligible class) has cls = cy = cx = -1, fg = 0, count = 0; fg = 1 marks
 *   a slot centred on (cy, cx).
 * csu_patch_locate: yx[i] = {y, x} of the r[i]-th pixel (raster order) of class cls[i] in image n[i], or {-1, -1}
 * when n, cls or r is out of range (r >= count).  The same device function as the draw's.
 *
 * csu_patch_warp: csu_augment_warp with a per-slot source.  The output is Ph x Pw; slot b reads image
 * n = record[b][0] (clamped to 0..N-1) with origin (ox, oy) = (record[b][5], record[b][4]) (clamped to +-2^24)
 * and mean[n].  table / ctrl are those of csu_augment_draw(cfg, B, Ph, Pw, ...): A, the B-spline field and the
 * noise index y Pw + x live in the patch frame.  The source position of output pixel p is (ox, oy) + A(p + d(p)):
 * s = A(p + d) is evaluated in fp32 in the patch frame as csu_augment_warp does, clamped to [-2 - o, L + 1 - o]
 * (constant border) or [-o, L - 1 - o] (replicate) per axis, floor / fraction / nearest rounding are taken there,
 * and the INTEGER origin is added to the integer tap coordinates: the result does not depend on where in a large
 * image the patch lies, and an integer table gives the exact slice.  Border rules (against the image n, not the
 * pool), image_fill, pad_label, mask modes, the intensity chain and the noise are csu_augment_warp's; with
 * origin 0 and Ph x Pw = H x W the two agree bit for bit.
 * ------------------------------------------------------------------------------------- */
#define CSU_PATCH_RECORD 16
int csu_patch_index(int N, int K, int max_h, const void* labels, const int64_t* meta, int32_t* rows, void* stream);
int csu_patch_draw(const void* labels, const int64_t* meta, const int32_t* rows, int N, int K, unsigned class_mask, int Ph,
                   int Pw, int B, int fg_slots, float p_fg, const int32_t* indices, const uint64_t* rng, unsigned site,
                   int32_t* record, void* stream);
int csu_patch_locate(const void* labels, const int64_t* meta, const int32_t* rows, int N, int K, int M, const int32_t* n,
                     const int32_t* cls, const int32_t* r, int32_t* yx, void* stream);
int csu_patch_warp(int B, int Ph, int Pw, int N, const void* pixels, const void* labels, const int64_t* meta,
                   const float* mean, const int32_t* record, const float* table, const float* ctrl, int spacing,
                   const uint64_t* rng, unsigned noise_site, int border, float image_fill, int pad_label, int mask_mode,
                   float* out_img, void* out_mask, void* stream);

/* ---------------------------------------------------------------------------------------
 * Tiled whole-image inference (csrc/tile.hip): sliding-window prediction of an H x W image with a
 * network of fixed S x S input, with test-time augmentation.  The reference has no counterpart.
 *   table: int32 (B, 6) on the device, one record per batch slot: {y0, x0, hflip, vflip, clockwise
 *      quarter turns 0..3 (applied after the flips, as csu_augment_batch), active}.  active = 0 marks
 *      a padding slot of a ragged last batch.  (y0, x0) is the tile's top-left pixel in the image.
 *   Pixel (y, x) of slot b's network input / output is tile pixel (ty, tx) = the stored-image pixel
 *   of the augmentation's mapping for (hflip, vflip, rot), i.e. image pixel (y0 + ty, x0 + tx).
 * csu_tile_gather: out fp32 (B, 3, S, S) from image uint8 (H, W, 3) (value / 255, an IEEE division)
 *      or fp32 (3, H, W) (copied).  Coordinates outside the image are clamped to its edge, so an
 *      image smaller than the tile is legal.  A padding slot gets slot 0's tile.
 * csu_tile_blend: canvas[k, y0 + ty, x0 + tx] += w1[ty] w1[tx] p_k for every active slot, network
 *      output pixel and class; canvas fp32 (K, H, W), w1 fp32 (S); pixels outside the canvas are
 *      dropped, padding slots contribute nothing.  form CSU_TILE_PROB: z fp32, K = 1, p = z.
 *      CSU_TILE_LOGITS: z fp32 or bf16 (upcast in registers), p = sigmoid(z) for K = 1, softmax over the
 *      classes for 2 <= K <= 32 (max-subtracted, fp32).  Element (b, k, pix) of z is at z[b s_b + k s_k
 *      + pix s_pix], pix = y S + x; class-last (s_k = 1) and NCHW (s_pix = 1) are read with vector
 *      loads, anything else per element; pad_ok as in csu_seg_ce_fwd.  1 <= B <= 128 per launch.
 *      Deterministic and order-preserving: no atomics; every canvas element receives its
 *      contributions one at a time in table order, starting from its value on entry -- so a tile
 *      list gives bitwise the same canvas however it is cut into launches.
 *      Region [ry0, ry1) x [rx0, rx1): the part of the canvas the launch covers -- the bounding box of
 *      the active slots' tiles, which the host knows from the table it made (0, 0, H, W: all of it).
 *      Canvas pixels outside the region (rounded outwards to the kernel's patches) are not updated.
 * csu_tile_finish: p = canvas / (ry[y] rx[x] n_tta) (ry (H), rx (W): the separable sum of the window
 *      over the tile plan); prob fp32 (K, H, W) and labels uint8 (H, W), either may be NULL (not
 *      both): label = p > 0.5 for K = 1, else argmax_k p with the lowest index winning a tie.
 * All three take the stream and are capturable (no allocation, no synchronisation).
 * CSU_E_ARG: a size < 1, B > 128 (blend), K < 1 or K > 32, an unknown src_kind, form or dtype, PROB with
 *      K != 1 or bf16, a stride < 1, an empty region or one outside the canvas, n_tta <= 0, a null pointer.
 * ------------------------------------------------------------------------------------- */
enum csu_tile_src { CSU_TILE_SRC_U8_HWC = 0, CSU_TILE_SRC_F32_CHW = 1 };
enum csu_tile_form { CSU_TILE_PROB = 0, CSU_TILE_LOGITS = 1 };
int csu_tile_gather(int B, int S, int H, int W, int src_kind, const void* image, const int* table, float* out,
                    void* stream);
int csu_tile_blend(int B, int S, int H, int W, int K, int form, int dtype, const void* z, long s_b, long s_k, long s_pix,
                   int pad_ok, const int* table, const float* w1, float* canvas, int ry0, int rx0, int ry1, int rx1,
                   void* stream);
int csu_tile_finish(int K, int H, int W, const float* canvas, const float* ry, const float* rx, float n_tta, float* prob,
                    void* labels, void* stream);

/* ---------------------------------------------------------------------------------------
 * Surface-distance metrics and an exact Euclidean distance transform (csrc/surface.hip).  The
 * definitions are medpy's (metric.binary.hd / hd95 / assd, and the surface Dice); the reference has no
 * counterpart.
 *   pred, target: label maps (B, H, W), contiguous, uint8 or int64 each (they may differ), read in place.
 *   For image b and class c (label value class0 + c; CSU_SURFACE_BINARY: C = 1 and a pixel is in the
 *   mask where its value is > 0) P and T are the two masks, dP and dT their borders: the mask pixels
 *   with at least one of the four edge neighbours outside the mask, everything beyond the image counting
 *   as outside.  The distance between pixels is sqrt(sy^2 dy^2 + sx^2 dx^2).  d1 = for every pixel of dP
 *   the distance to the nearest pixel of dT, d2 the same from dT to dP.
 * csu_surface_metrics: out[(b out_classes + out_c0 + c) 6 ..] = fp64 {hd, hd95, assd, nsd, |dP|, |dT|}:
 *      hd = max(max d1, max d2); hd95 = the `percentile`-th percentile of the pooled d1 and d2 with linear
 *      interpolation (sorted v, h = (n - 1) q / 100, v[floor h] + (h - floor h)(v[floor h + 1] - v[floor h]));
 *      assd = (mean d1 + mean d2) / 2; nsd = (#{d1 <= tolerance} + #{d2 <= tolerance}) / (|dP| + |dT|).
 *      Where P or T is empty the first four are NaN.  out_classes / out_c0 let a caller fill a
 *      (B, out_classes, 6) tensor in class chunks.
 *      sy == sx: squared index distances in int32 (exact), scaled by s^2 in fp64, and d <= tolerance decided
 *      as d2 s^2 <= tolerance^2; otherwise squared distances in fp32 (sy^2, sx^2 rounded to fp32).  Square
 *      roots, sums and the percentile in fp64.  No floating-point atomics: block partials are combined in
 *      a fixed order, so results are bitwise repeatable and do not depend on B, C or the chunking.
 *      Workspace: csu_surface_workspace(B, C, H, W) bytes = B C (12 H W + 40 H) + O(B C) for tables, each
 *      part rounded up to 256: per (image, class) two uint16 (H, W) column-distance fields, a list of up
 *      to 2 H W 32-bit keys (one per border pixel), per-row partials and 4 x 2 x 256 histogram bins.
 * csu_edt: out fp32 (B, H, W) = for every non-zero pixel of mask (B, H, W) the distance to the nearest
 *      zero pixel, 0 at the zero pixels (scipy.ndimage.distance_transform_edt with sampling = (sy, sx));
 *      inf everywhere in an image without a zero pixel.  Workspace csu_edt_workspace(B, H, W) = 2 B H W bytes.
 * Both take the stream and are capturable (no allocation, no synchronisation).
 * CSU_E_ARG: a size < 1, H or W > 32767, C > 32, B C 2 > 65535 (edt: B > 65535), an unknown mode or dtype,
 *      BINARY with C != 1, a spacing that is not positive and finite, tolerance < 0, percentile outside
 *      [0, 100], classes outside the out rows, a null pointer.  CSU_E_WORKSPACE: workspace too small.
 * ------------------------------------------------------------------------------------- */
enum csu_surface_dtype { CSU_SURFACE_U8 = 0, CSU_SURFACE_I64 = 1 };
enum csu_surface_mode { CSU_SURFACE_LABELS = 0, CSU_SURFACE_BINARY = 1 };
size_t csu_surface_workspace(int B, int C, int H, int W);
int csu_surface_metrics(int B, int C, int H, int W, int mode, int class0, int pred_dtype, const void* pred,
                        int target_dtype, const void* target, double sy, double sx, double tolerance, double percentile,
                        void* workspace, size_t ws_bytes, double* out, int out_classes, int out_c0, void* stream);
size_t csu_edt_workspace(int B, int H, int W);
int csu_edt(int B, int H, int W, int dtype, const void* mask, double sy, double sx, void* workspace, size_t ws_bytes,
            float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Signed distance maps of a label map's classes (csrc/surface.hip): phi of the boundary loss
 * (csu_seg_bd_*), Kervadec's one_hot2dist; the reference has no counterpart.
 *   labels: (B, H, W), contiguous, CSU_SURFACE_U8 or CSU_SURFACE_I64, read in place.  For image b and class c
 *   (label value class0 + c) M is the set of pixels that hold the value.  A pixel with any other value, an
 *   ignore_index included, is outside every class.  Beyond the image there is nothing: the image edge is
 *   no border (unlike the surface metrics above).  With S = diag(sy, sx):
 *      M empty or the whole image:  phi = 0 everywhere;
 *      x not in M:  phi(x) =   min over y in M     of |S (x - y)|;
 *      x in M:      phi(x) = -(min over y not in M of |S (x - y)| - min(sy, sx)),  0 on the inner border;
 *   with unit spacing edt(neg) neg - (edt(pos) - 1) pos.  clip > 0: phi is clamped to [-clip, clip] (and the row
 *   search stops at that radius); clip < 0: none.
 *   out fp32 (B, out_classes, H, W), class c written at plane out_c0 + c.
 * The column pass of the transform above runs twice per (image, class), with the pixels on and off the
 * class as sites, into two uint16 fields; one row pass stages the row of both in LDS and searches, for
 * every pixel, the field of the other side.  sy == sx: int32 index distances (exact); otherwise fp32.  No
 * atomics, no synchronisation, capturable; results are bitwise repeatable and do not depend on B, C or
 * the chunking.  Workspace csu_signed_distance_workspace(B, C, H, W) = 4 B C H W bytes rounded up to 256.
 * CSU_E_ARG: a size < 1, H or W > 16383 (the rows of two fields fill 64 KiB of LDS), C > 32, B C 2 > 65535,
 *      an unknown dtype, a spacing that is not positive and finite, clip 0 / inf / NaN, classes outside the
 *      out planes, a null pointer.  CSU_E_WORKSPACE: workspace too small.
 * ------------------------------------------------------------------------------------- */
size_t csu_signed_distance_workspace(int B, int C, int H, int W);
int csu_signed_distance(int B, int C, int H, int W, int class0, int dtype, const void* labels, double sy, double sx,
                        double clip, void* workspace, size_t ws_bytes, float* out, int out_classes, int out_c0,
                        void* stream);

/* ---------------------------------------------------------------------------------------
 * Connected-component labelling and the component rules of segmentation post-processing
 * (csrc/components.hip); the reference has no counterpart.
 *   labels: a label map (B, H, W), contiguous, CSU_SURFACE_U8 or CSU_SURFACE_I64, read in place.  Value 0 is
 *   background.  Two neighbouring pixels belong to one component iff they hold the same value and are
 *   adjacent: `connectivity` CSU_CC_4 (edges) or CSU_CC_8 (edges and corners) for the non-zero values,
 *   always 4-adjacency for value 0 (the background components come out of the same pass, in
 *   scipy.ndimage.binary_fill_holes' convention).  All values are labelled in one pass.
 * csu_ccl: each output may be NULL, not all three.
 *      comp  int32 (B, H, W): 0 at the zero pixels, elsewhere the component's number within its image,
 *            1 .. N in raster order of the components' first pixels (for a binary map: scipy.ndimage.label with
 *            the 3 x 3 all-ones structure for CSU_CC_8, the cross for CSU_CC_4).
 *      area  int32 (B, H, W): every pixel, the zero ones included, holds the pixel count of its component.
 *      count int32 (B): N, the number of non-zero components of each image.
 *      Workspace: csu_ccl_workspace(B, H, W) bytes = 3 x 4 B H W + 4 B ceil(H W / 4096), each of the four
 *      parts rounded up to 256: parents, {count, non-zero bit, touches-the-border bit} per root, numbers,
 *      and the root counts of 4096-pixel chunks.  The touches-border field stays in the workspace.
 * csu_cc_filter: out (B, H, W) of the labels' dtype = the map after three steps, each applied to the map the
 *      step before produced.  out may be the very buffer of labels (no other overlap).
 *      1. fill_holes != 0: a hole is a zero component that does not touch the image border, of at most
 *         max_hole_size pixels (-1: any size); it takes the value of the pixel left of its first pixel in
 *         raster order, unless that value is >= num_classes (then it stays).
 *      2. every component of a class c with fewer than min_size[c] pixels becomes 0 (min_size NULL: none).
 *      3. for every class c with bit c of keep_largest set, all of its components in an image become 0 but
 *         the largest one; ties go to the lowest component number.
 *      Classes are the values 1 .. num_classes - 1; min_size has num_classes entries (entry 0 unused).  For
 *      num_classes = 1 the only class is the value 1 and entry 0 / bit 0 are its rules.  Values >=
 *      num_classes (an ignore value) form components like any other, are never holes, and no rule touches
 *      them.  Steps 2 and 3 work on a fresh labelling of the filled map: filling can join components.
 *      Workspace: csu_cc_filter_workspace(B, H, W) bytes = 2 x 4 B H W + 256 B, each of the three parts
 *      rounded up to 256: parents, per-root fields, and a 64-bit (area, ~first pixel) key per image and class.
 * Results are unique by definition (roots are minimum pixel indices, numbers are ranks): bitwise repeatable,
 * independent of B and of any chunking.  Integer atomics only.  Both take the stream and are capturable
 * (no allocation, no synchronisation, nothing returned to the host); no workgroup waits for another.
 * CSU_E_ARG: a size < 1, H or W > 32767, B > 65535 or B ceil(H / 64) ceil(W / 64) > 2^23 (the grid of the tile
 *      pass), a connectivity other than 4 or 8, an unknown dtype, num_classes outside 1..32, a negative min_size,
 *      max_hole_size < -1, null labels / workspace / out, all of comp, area, count null.
 *      CSU_E_WORKSPACE: workspace too small.
 * ------------------------------------------------------------------------------------- */
enum csu_cc_connectivity { CSU_CC_4 = 4, CSU_CC_8 = 8 };
size_t csu_ccl_workspace(int B, int H, int W);
int csu_ccl(int B, int H, int W, int dtype, const void* labels, int connectivity, void* workspace, size_t ws_bytes,
            int* comp, int* area, int* count, void* stream);
size_t csu_cc_filter_workspace(int B, int H, int W);
int csu_cc_filter(int B, int H, int W, int dtype, const void* labels, int connectivity, int num_classes,
                  const int* min_size, unsigned keep_largest, int fill_holes, int max_hole_size, void* workspace,
                  size_t ws_bytes, void* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Plain-UNet BatchNorm2d (+ ReLU) and MaxPool2d(2) on NHWC rows (DoubleConv / Down,
 * train_unet_segmentation.py unet:177-204; replaces F.batch_norm + F.relu + F.max_pool2d there).
 * x, y: M = B*H*W rows of C channels (C % 8 == 0), dtype bf16 or f32 (y and dx in x's dtype).
 * training: batch statistics (biased variance) -> save = (mean[C], rstd[C]); running_mean /
 * running_var (may both be NULL) updated with `momentum` and the unbiased variance; else the
 * running statistics normalise.  relu != 0 fuses the following ReLU (backward masks by y > 0,
 * recomputed).  Deterministic (fixed-order reductions); workspace csu_bn_workspace(M, C) bytes.
 * ------------------------------------------------------------------------------------- */
size_t csu_bn_workspace(long M, int C);
int csu_bn_relu_fwd(long M, int C, int dtype, const void* x, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, int training, int relu,
                    float* save, void* y, void* workspace, size_t ws_bytes, void* stream);
/* dx, dgamma, dbeta (either may be NULL) from dy (gdtype) and the forward's save */
int csu_bn_relu_bwd(long M, int C, int dtype, const void* x, const float* gamma, const float* beta, const float* save,
                    int training, int relu, int gdtype, const void* dy, void* dx, float* dgamma, float* dbeta,
                    void* workspace, size_t ws_bytes, void* stream);
/* MaxPool2d(2) of NHWC x (B, H, W, C) -> y (B, H/2, W/2, C); the backward writes every dx element
 * of the pooled 2x2 windows (the first maximum in torch's scan order gets dy, NaN wins); rows /
 * columns past 2*(H/2), 2*(W/2) are not written. */
int csu_maxpool2_fwd(int B, int H, int W, int C, int dtype, const void* x, void* y, void* stream);
int csu_maxpool2_bwd(int B, int H, int W, int C, int dtype, const void* x, int gdtype, const void* dy, void* dx,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CSU_H_ */
