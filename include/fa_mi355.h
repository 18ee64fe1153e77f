/*
 * fa_mi355.h - C ABI of libfa_mi355.so: the MI355X (gfx950 / CDNA4) fused attention path.
 *
 * This is the drop-in boundary for the reference's private extension module
 * `flash_attn_v100_cuda` (ai-bond/flash-attention-v100).  Each entry point replaces one
 * op of that module; the reference prototypes are cited per function below
 * (include/mha.h and kernel/fused_mha_api.cpp of the reference).
 *
 * Conventions
 *   - plain C: raw device pointers, sizes, strides IN ELEMENTS, POD structs, an explicit
 *     HIP stream (void* == hipStream_t).  No torch / ATen types.
 *   - never allocates: the caller owns every buffer (outputs, workspaces).  Workspace
 *     sizes come from the *_workspace_bytes() queries.
 *   - never throws: returns FA_OK (0) or a negative fa_status; the message of the last
 *     failure on the calling thread is returned by fa_last_error().
 *   - inputs are borrowed; outputs are written in place; k_cache / v_cache are mutated
 *     in place by fa_fwd_kvcache (reference: kernel/fused_mha_forward_kvcache.cu:134-141).
 *   - launches are asynchronous on `stream`; no host synchronisation inside.
 *   - Tensor layouts are described by strides, so the (B,S,H,D) tensors of the Python API
 *     are passed as they are (the reference permutes + copies to (B,H,S,D) first,
 *     flash_attn_v100/flash_attn_interface.py:36-53).
 */
#ifndef FA_MI355_H
#define FA_MI355_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_ABI_VERSION 4   /* 2: fa_bwd / fa_varlen_bwd skip outputs passed as NULL; 3: fa_params::flags (was reserved0);
                              4: fa_params::q_descale, fa_params::o_dtype (fp8-e4m3 q in fa_fwd / fa_varlen_fwd) */

/* fa_params::flags.  The reference drops a window of >= seqlen_k keys before anything else (fused_mha_forward.cu:343-352); so
 * do the five ops.  With seqlen_q > seqlen_k that also drops right windows that still hide keys from the first rows - the
 * mask of a context-parallel shard (all queries over a slice of the keys).  FA_FLAG_KEEP_WINDOW keeps such a window; it is an
 * extension for this library's own sharding wrapper and never set by the drop-in Python API. */
#define FA_FLAG_KEEP_WINDOW 1
/* fa_bwd / fa_varlen_bwd.  A dK/dV launch with fewer workgroups than the GPU has room for (batch x kv-heads x 128-key blocks: GQA at
 * micro-batch 1, short-key cross-attention) divides the query rows of each key block over several workgroups and adds their
 * 16-bit partial dK / dV in fp32 (deterministic; needs the workspace fa_bwd_workspace_bytes() reports).  dK / dV then differ in
 * the last bit from the one-workgroup-per-key-block result.  FA_FLAG_NO_DKV_SPLIT keeps one workgroup per key block. */
#define FA_FLAG_NO_DKV_SPLIT 2
/* fa_bwd, opt-in, measured at break-even over short runs and 5 % slower sustained (profiles/r06_ds_handoff.txt): where the dense D = 128 backward would run its two generated
 * kernels and all three gradients are requested, the dK/dV kernel hands its 16-bit dS tiles to a one-GEMM dQ kernel through the
 * workspace (2 bytes per (query, key) pair and head: fa_bwd_workspace_bytes() reports it) instead of dQ recomputing S and dP.
 * Same results up to the order of fp32 additions.  Ignored where it does not apply. */
#define FA_FLAG_DS_HANDOFF 4
/* fa_fwd, opt-in, measured a net loss at the shapes it was built for (profiles/r06_fwd_split.txt).  A causal-like dense D = 128 launch
 * whose 256-row query blocks all get a compute unit at once (batch x heads x ceil(Sq / 256) <= the CU count: micro-batch-1 training,
 * batch-1 prefill, a tensor-parallel shard) runs as long as its heaviest block; with this flag and the workspace
 * fa_fwd_workspace_bytes() reports, the heavy blocks' key ranges are cut into 2 - 4 parts whose fp32 partial outputs a merge kernel
 * combines (deterministic; out / LSE equal the unsplit result up to the order of fp32 additions).  Ignored where it does not apply. */
#define FA_FLAG_FWD_KEY_SPLIT 8
/* fa_fwd_kvcache_tree only: a tree block (fa_tree_params below) accompanies the call.  The caller sets it whenever it passes one, so
 * that fa_fwd_kvcache_workspace_bytes() - which sees fa_params alone - answers for the route a tree call takes (always the decode
 * kernels).  The flag without a tree block, a tree block without the flag, and the flag on any other op are
 * FA_ERR_INVALID_ARGUMENT. */
#define FA_FLAG_TREE_MASK 16

typedef enum fa_dtype {
    FA_FP16 = 0,      /* IEEE half */
    FA_BF16 = 1,      /* bfloat16 */
    FA_FP8_E4M3 = 2,  /* OCP e4m3fn: k/v of fa_fwd_kvcache and of paged fa_varlen_fwd; q, k and v together in fa_fwd /
                         fa_varlen_fwd (forward only, 16-bit o of fa_params::o_dtype) */
    FA_FP32 = 3       /* IEEE single: weights / residuals of the norm ops, logits of fa_cross_entropy */
} fa_dtype;

typedef enum fa_status {
    FA_OK = 0,
    FA_ERR_INVALID_ARGUMENT = -1,   /* a TORCH_CHECK of the reference would have fired */
    FA_ERR_UNSUPPORTED = -2,        /* valid request this build has no kernel for */
    FA_ERR_LAUNCH = -3,             /* HIP runtime reported an error */
    FA_ERR_NO_DEVICE = -4
} fa_status;

/*
 * One parameter block serves all five ops; each op reads the fields that apply to it
 * and ignores the rest (zero-initialise the struct).  Index conventions:
 *   element (b, i, h, d) of q  =  q[b*q_batch_stride + i*q_row_stride + h*q_head_stride + d]
 *   (last dimension contiguous).  Varlen: b*batch_stride is replaced by cu_seqlens[b]*row_stride.
 *   Paged K/V: logical key j of batch b lives in page block_table[b*block_table_batch_stride
 *   + j / page_block_size], row j % page_block_size; k_batch_stride is then the PAGE stride.
 */
typedef struct fa_params {
    /* ---- forward tensors ---- */
    const void* q;            /* [B, Sq, Hq, D]  (varlen: [Tq, Hq, D]) */
    const void* k;            /* [B, Sk, Hk, D]  (varlen: [Tk, Hk, D]; paged: [nblk, page, Hk, D]) */
    const void* v;
    void*       o;            /* same shape as q */
    float*      lse;          /* dense/kvcache [B, Hq, Sq]; varlen [Hq, Tq]  (natural log) */
    int64_t q_batch_stride, q_row_stride, q_head_stride;
    int64_t k_batch_stride, k_row_stride, k_head_stride;
    int64_t v_batch_stride, v_row_stride, v_head_stride;
    int64_t o_batch_stride, o_row_stride, o_head_stride;
    int64_t lse_batch_stride, lse_head_stride;   /* row stride is 1 */

    /* ---- backward tensors (fa_bwd / fa_varlen_bwd) ---- */
    const void* dout;         /* same layout family as o, own strides */
    void*       dq;
    void*       dk;
    void*       dv;
    float*      softmax_d;    /* rowsum(dO * O), same layout as lse; REQUIRED (written) */
    int64_t do_batch_stride, do_row_stride, do_head_stride;
    int64_t dq_batch_stride, dq_row_stride, dq_head_stride;
    int64_t dk_batch_stride, dk_row_stride, dk_head_stride;
    int64_t dv_batch_stride, dv_row_stride, dv_head_stride;

    /* ---- sizes ---- */
    int32_t batch;
    int32_t nheads_q;
    int32_t nheads_k;
    int32_t seqlen_q;         /* dense: Sq; varlen: max_seqlen_q; kvcache: Tq */
    int32_t seqlen_k;         /* dense: Sk; varlen: max_seqlen_k; kvcache: cache capacity
                                 (S_max, or pages_per_seq * page_block_size when paged) */
    int32_t head_dim;         /* kernel width: 64, 128 or 256 */
    int32_t dtype;            /* fa_dtype of q/o/dout/dq/dk/dv */
    int32_t kv_dtype;         /* fa_dtype of k/v (== dtype, or FA_FP8_E4M3 for fa_fwd_kvcache) */

    /* ---- attention options ---- */
    float   softmax_scale;
    float   softcap;          /* 0 = off.  s = softcap * tanh(s / softcap), applied AFTER ALiBi
                                 (reference order, include/mat_mul.h:113-116) */
    int32_t is_causal;        /* bottom-right aligned: key j visible iff j - (Sk - Sq) <= i */
    int32_t window_left;      /* -1 = unbounded */
    int32_t window_right;     /* -1 = unbounded */
    const float* alibi_slopes;      /* fp32 [Hq] or [B, Hq]; NULL = off */
    int64_t alibi_batch_stride;     /* 0 for [Hq] */

    /* ---- dropout (Philox-4x32-10, reference stream: include/softmax.h:97-104) ---- */
    float    p_dropout;       /* probability of dropping */
    uint64_t philox_seed;
    uint64_t philox_offset;
    void*    dmask;           /* optional [B,Hq,Sq,Sk] (varlen: [Tq,Hq,max_sk]) of `dtype`:
                                 +1 kept / -1 dropped; NULL = not requested */

    /* ---- varlen ---- */
    const int32_t* cu_seqlens_q;    /* [B+1] */
    const int32_t* cu_seqlens_k;    /* [B+1] */
    const int32_t* seqused_k;       /* [B] or NULL */
    int32_t        total_q;         /* Tq (varlen) */
    int32_t        total_k;         /* Tk (varlen, non-paged) */

    /* ---- paged KV ---- */
    const int32_t* block_table;     /* [B, max_blocks] or NULL */
    int64_t        block_table_batch_stride;
    int32_t        page_block_size;   /* tokens per page: any multiple of 16 */
    int32_t        head_dim_v;      /* valid columns of every row (multiple of 8, <= head_dim); 0 = head_dim.
                                       Columns [head_dim_v, head_dim) are read as zero and never written: odd
                                       head dims (40, 80, 96, 192 ...) run on the next kernel width without
                                       padded copies of the tensors. */

    /* ---- KV cache (fa_fwd_kvcache) ---- */
    const int32_t* cache_seqlens;   /* [B] or NULL (=0) */
    const int32_t* cache_batch_idx; /* [B] or NULL */
    const int32_t* cache_leftpad;   /* [B] or NULL */
    const void*    k_new;           /* [B, T_new, Hk, D] of `dtype`, or NULL */
    const void*    v_new;
    int64_t knew_batch_stride, knew_row_stride, knew_head_stride;
    int64_t vnew_batch_stride, vnew_row_stride, vnew_head_stride;
    int32_t        seqlen_new;      /* T_new */
    int32_t        rotary_dim;      /* 0 = no rotary */
    const void*    rotary_cos;      /* [seqlen_ro, rotary_dim/2] of `dtype` */
    const void*    rotary_sin;
    int32_t        rotary_interleaved;
    int32_t        seqlen_ro;
    float          k_descale;       /* fp8 cache: value = code * descale (1.0 otherwise) */
    float          v_descale;

    /* ---- split-KV (decode) ---- */
    int32_t num_splits;             /* 0 = heuristic, 1 = no split */
    int32_t flags;                  /* FA_FLAG_* bits, 0 for the reference's semantics (unknown bits are rejected) */
    void*   workspace;              /* >= fa_*_workspace_bytes(params) bytes, or NULL if 0 */
    size_t  workspace_bytes;

    /* ---- fp8-e4m3 q, k, v (ABI 4: fa_fwd / fa_varlen_fwd with dtype == kv_dtype == FA_FP8_E4M3) ----
     * Both products run on the block-scaled e4m3 matrix pipe; value = code * descale for each of q, k, v (k_descale and
     * v_descale above).  A descale of 0 means 1.0; a negative or non-finite one is FA_ERR_INVALID_ARGUMENT.
     * q_descale * k_descale joins softmax_scale, v_descale the final normalisation.  Head dims 64 and 128 (head_dim_v: a
     * multiple of 16), causal / window masks, GQA / MQA, dense and varlen (non-paged); ALiBi, softcap, dropout, paged K/V
     * and head dims above 128 are FA_ERR_UNSUPPORTED.  No backward: fa_bwd / fa_varlen_bwd / fa_fwd_kvcache reject fp8 q. */
    float   q_descale;              /* fp8 q: value = code * q_descale (0 = 1.0); ignored otherwise */
    int32_t o_dtype;                /* fp8 q: fa_dtype of o, FA_FP16 or FA_BF16; ignored for 16-bit q (o has `dtype`) */
} fa_params;

/* ABI self-description (checked by the Python ctypes mirror at load time). */
int         fa_abi_version(void);
size_t      fa_params_size(void);
const char* fa_last_error(void);
const char* fa_build_info(void);           /* arch, compiler, kernel variants */


/* Workspace queries (bytes; 0 = none needed).  fa_fwd_workspace_bytes covers fa_fwd (non-zero only with FA_FLAG_FWD_KEY_SPLIT on one-wave causal launches) and fa_varlen_fwd: non-zero
 * when the call is a decode step issued through the varlen op (every sequence brings the same <= 32 query tokens, paged
 * K / V) or a mixed batch whose sequences are mostly short (decode sequences next to a prefill chunk) - with the workspace
 * the split-KV decode kernels serve the short sequences, without it the general kernel serves everything (same results). */
size_t fa_fwd_workspace_bytes(const fa_params* p);
/* fa_bwd_workspace_bytes: the row-statistics planes of the hand-scheduled D = 128 dK/dV kernel (2 x rows x heads x 4 bytes) and, for
 * dK/dV launches smaller than the GPU (see FA_FLAG_NO_DKV_SPLIT), fp32 partial dK / dV slabs behind them.  A smaller or NULL workspace
 * is legal: the kernels that need no workspace run (same results up to the order of fp32 additions).
 * One query serves fa_bwd AND fa_varlen_bwd: pass the struct EXACTLY as it goes into the op - cu_seqlens_q / cu_seqlens_k select the
 * packed sizing and split decision, and fa_bwd itself ignores them (a dense caller that recycles a struct must clear the varlen
 * fields before the query, or the sizes answer the varlen op; the `workspace_bytes` guard of the ops keeps a mismatch safe - the
 * split is then dropped or the slabs go unused - but not fast).  The split decision reads the CU count of the CURRENT device:
 * query on the device the op will be launched on. */
size_t fa_bwd_workspace_bytes(const fa_params* p);
size_t fa_fwd_kvcache_workspace_bytes(const fa_params* p);

/*
 * fa_fwd - dense forward.  Replaces `flash_attn_v100_cuda.fwd`
 *   reference: include/mha.h:27-41, kernel/fused_mha_forward.cu:301-432
 *   writes o, lse (and dmask when requested and p_dropout > 0).
 */
int fa_fwd(const fa_params* p, void* stream);

/*
 * fa_bwd - dense backward.  Replaces `flash_attn_v100_cuda.bwd`
 *   reference: include/mha.h:67-87, kernel/fused_mha_backward.cu:577-721
 *   reads dout, q, k, v, o, lse; writes dq, dk, dv, softmax_d.  Deterministic
 *   (no atomics).  GQA: dk/dv are summed over the q-heads of each kv-head in-kernel.
 *   Gradients the caller does not need are skipped: dq == NULL -> the dQ kernel does not run;
 *   dk == dv == NULL -> the dK/dV kernel does not run (autograd's needs_input_grad; softmax_d is
 *   always written).  The same holds for fa_varlen_bwd.
 */
int fa_bwd(const fa_params* p, void* stream);

/*
 * fa_varlen_fwd - packed variable-length forward (optionally paged K/V).
 *   Replaces `flash_attn_v100_cuda.varlen_fwd`
 *   reference: include/mha.h:116-139, kernel/fused_mha_forward_varlen.cu:371-566
 */
int fa_varlen_fwd(const fa_params* p, void* stream);

/*
 * fa_varlen_bwd - packed variable-length backward.  Replaces `flash_attn_v100_cuda.varlen_bwd`
 *   reference: include/mha.h:170-195, kernel/fused_mha_backward_varlen.cu:636-807
 */
int fa_varlen_bwd(const fa_params* p, void* stream);

/*
 * fa_fwd_kvcache - append new K/V (+RoPE) into the cache, then attention of q over the
 *   cache (decode / chunked prefill).  Replaces `flash_attn_v100_cuda.fwd_kvcache`
 *   reference: include/mha.h:224-245, kernel/fused_mha_forward_kvcache.cu:416-652
 */
int fa_fwd_kvcache(const fa_params* p, void* stream);

/*
 * Extension block of the *_ext entry points (additive: fa_params and FA_ABI_VERSION are unchanged).
 *
 * Attention sinks: one learned logit s_h per query head joins the softmax denominator and carries no value,
 *   out_i = sum_j e^{x_ij} v_j / (e^{s_h} + sum_j e^{x_ij}),   LSE_i = log(e^{s_h} + sum_j e^{x_ij}),
 * x_ij the final score (softmax_scale q.k, then softcap, then ALiBi).  The LSE written is the sink-inclusive one; a row
 * without visible keys gives out = 0, LSE = s_h; a sink of -inf is no sink (bit for bit).  The backward's dq / dk / dv
 * follow from the sink-inclusive LSE; dsinks_h = -sum_{b,i} exp(s_h - LSE_{b,h,i}) D_{b,h,i} (D = rowsum(dO o O)) is a
 * fixed-order reduction (bitwise repeatable, no atomics).
 * Not covered (FA_ERR_UNSUPPORTED): fp8-e4m3 q/k/v and dropout.  The workspace queries are unchanged.
 */
typedef struct fa_ext_params {
    size_t       struct_size;  /* sizeof(fa_ext_params) as the caller compiled it */
    const float* sinks;        /* [nheads_q] fp32 sink logits (natural-log units), contiguous; NULL = none */
    float*       dsinks;       /* fa_bwd_ext / fa_varlen_bwd_ext: [nheads_q] fp32 gradient, written (not accumulated); NULL = not wanted */
} fa_ext_params;

/* The ABI-4 ops with an extension block.  ext == NULL, or sinks == dsinks == NULL: exactly the op without _ext. */
int fa_fwd_ext(const fa_params* p, const fa_ext_params* ext, void* stream);
int fa_varlen_fwd_ext(const fa_params* p, const fa_ext_params* ext, void* stream);
int fa_fwd_kvcache_ext(const fa_params* p, const fa_ext_params* ext, void* stream);
int fa_bwd_ext(const fa_params* p, const fa_ext_params* ext, void* stream);
int fa_varlen_bwd_ext(const fa_params* p, const fa_ext_params* ext, void* stream);

/*
 * Tree attention masks for speculative decoding (additive, like the block above: fa_params and FA_ABI_VERSION are unchanged).
 *
 * The call brings T_q = seqlen_q query tokens per sequence, 2 <= T_q <= 64: the nodes of a draft tree.  Their K / V are appended
 * by the same call (k_new / v_new with seqlen_new == T_q) or already sit at the end of the cache (seqlen_new == 0).  With
 * seqlen_k = cache_seqlens[b] + seqlen_new and off = seqlen_k - T_q:
 *   - key j < off (the committed cache) is visible to every query row;
 *   - key off + c, 0 <= c < T_q, is visible to row t iff bit (c & 31) of word (c >> 5) of mask[b, t] is set.
 * The mask REPLACES the causal rule (is_causal is accepted and has no further effect); it need not be topologically ordered nor
 * contain the diagonal.  A row without a visible key gives out = 0 and LSE = -inf (with attention sinks: LSE = s_h).
 * With seqlen_new == 0 the nodes are the LAST T_q keys of the cache, so the caller passes cache_seqlens[b] >= T_q (lengths
 * live on the device and are not checked): a shorter cache gives off < 0, the bits c < -off then name keys that do not exist
 * and are ignored, nothing is read out of bounds.
 * Positions: node t sits at position cache_seqlens[b] + cache_leftpad[b] + depths[b, t] for the in-kernel RoPE of q and of the new
 * k, while its cache SLOT stays cache_seqlens[b] + t.  depths is required when rotary_dim > 0 and ignored otherwise.
 * Works with softcap, attention sinks, GQA / MQA, paged and contiguous caches, cache_batch_idx, cache_leftpad, fp8-e4m3 caches,
 * num_splits and every head width of fa_fwd_kvcache.  Every tree call runs on the split-KV decode kernels (32 packed rows per
 * workgroup); set FA_FLAG_TREE_MASK in fa_params::flags for the call AND for its fa_fwd_kvcache_workspace_bytes() query.
 * Windows must be off (window_left == window_right == -1: FA_ERR_INVALID_ARGUMENT otherwise).
 * Out of scope: ALiBi with a tree (FA_ERR_UNSUPPORTED: its distance term needs tree positions), tree masks through the varlen
 * op's decode route, T_q > 64, and any backward.
 */
typedef struct fa_tree_params {
    size_t          struct_size;          /* sizeof(fa_tree_params) as the caller compiled it */
    const uint32_t* mask;                 /* [B, T_q, mask_words] (or [T_q, mask_words]) visibility words, 4-byte aligned; NULL = no tree */
    int64_t         mask_batch_stride;    /* in words; 0 = one tree for the whole batch */
    int32_t         mask_words;           /* ceil(T_q / 32): 1 or 2 */
    const int32_t*  depths;               /* [B, T_q] (or [T_q]) node depths, 4-byte aligned; NULL = none (no rotary) */
    int64_t         depths_batch_stride;  /* in elements; 0 = one depth array for the whole batch */
} fa_tree_params;

/* fa_fwd_kvcache_ext with a tree block.  tree == NULL or tree->mask == NULL: exactly fa_fwd_kvcache_ext. */
int fa_fwd_kvcache_tree(const fa_params* p, const fa_ext_params* ext, const fa_tree_params* tree, void* stream);
size_t fa_tree_params_size(void);

/*
 * fa_merge_states - combine attention computed over DISJOINT key sets into attention over their union (additive, like the blocks
 * above: fa_params and FA_ABI_VERSION are unchanged).
 *
 * Every part s is the (o, lse) pair a forward op of this library wrote for the same queries over its own keys.  Per (batch, row,
 * head), in fp32:
 *   LSE = logsumexp_s(lse_s),   out = sum_s exp(lse_s - LSE) out_s.
 * A part whose lse_s is -inf (no visible key) contributes nothing, even where its out_s holds NaN; if every part is -inf the row
 * gives out = 0 and LSE = -inf.  With exactly one finite part the row's out and LSE are that part's, bit for bit.
 * With attention sinks, pass the sink to ONE of the forward calls only: its sink-inclusive LSE then makes the merged LSE the
 * sink-inclusive LSE of the whole problem (a sink in two parts would be counted twice).
 * Use: shared-prefix ("cascade") decode - one fa_fwd of all queries of a batch over the common prefix, one fa_fwd_kvcache over
 * each sequence's own tokens, then this merge - and the per-step reduction of context / ring parallelism.
 * Element (b, i, h, d) of a part's o = o[b*o_batch_stride + i*o_row_stride + h*o_head_stride + d] (strides in elements, the last
 * dimension contiguous); element (b, h, i) of its lse = lse[b*lse_batch_stride + h*lse_head_stride + i*lse_row_stride].  The
 * three explicit LSE strides let one call take the [1, H, B*T] LSE of an fa_fwd over all B*T query rows as one sequence (batch
 * stride T, head stride B*T, row stride 1) next to fa_fwd_kvcache's [B, H, T] LSE, or a row-major [B, T, H] one, without a copy.
 * One kernel launch on `stream`: byte movement (16-byte loads and stores where every o base and stride is a multiple of 16 bytes,
 * 8-byte ones where they are multiples of 8), no atomics, no workspace, bitwise repeatable.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; n_parts outside 2 .. FA_MERGE_MAX_PARTS; a NULL o or lse;
 * head_dim not a multiple of 8 or above 256; a dtype other than FA_FP16 / FA_BF16; negative sizes; an lse that is not 4-byte
 * aligned; an o base or stride that is not a multiple of 8 bytes; an output o or lse whose base equals a part's (no in-place
 * merge).  Other overlap between the output and a part is not detected and not supported.
 */
#define FA_MERGE_MAX_PARTS 8

typedef struct fa_merge_state {
    void*   o;                 /* [batch, seqlen, nheads, head_dim] of fa_merge_params::dtype (parts: read only) */
    float*  lse;               /* fp32 [batch, nheads, seqlen], natural log (parts: read only) */
    int64_t o_batch_stride, o_row_stride, o_head_stride;
    int64_t lse_batch_stride, lse_head_stride, lse_row_stride;
} fa_merge_state;

typedef struct fa_merge_params {
    size_t         struct_size;   /* sizeof(fa_merge_params) as the caller compiled it */
    int32_t        n_parts;       /* 2 .. FA_MERGE_MAX_PARTS */
    int32_t        batch, seqlen, nheads;
    int32_t        head_dim;      /* a multiple of 8, <= 256 */
    int32_t        dtype;         /* FA_FP16 or FA_BF16: every part's o and the output o */
    fa_merge_state parts[FA_MERGE_MAX_PARTS];
    fa_merge_state out;           /* written */
} fa_merge_params;

int    fa_merge_states(const fa_merge_params* m, void* stream);
size_t fa_merge_params_size(void);

/*
 * fa_rotary - standalone rotary position embedding (additive, like the blocks above: fa_params and FA_ABI_VERSION are unchanged).
 *
 * out = rope(x, pos) for every (batch, row, head) of x, with the pair rule and the arithmetic of fa_fwd_kvcache's in-kernel RoPE
 * (fp32 math, c = cos[pos, t], s = sin[pos, t], the result rounded once to the 16-bit io type):
 *   interleaved:  (x[2t], x[2t+1])         -> (x0 c - x1 s, x0 s + x1 c)      t < rotary_dim / 2
 *   otherwise:    (x[t], x[t+rotary_dim/2]) -> likewise                         (GPT-NeoX)
 * conjugate != 0 negates s first (exactly): the inverse rotation, which is also the backward of the op.
 * Element (b, i, h, d) of x = x[b*x_batch_stride + i*x_row_stride + h*x_head_stride + d] (strides in elements, the last dimension
 * contiguous); with cu_seqlens the tensor is packed, [total_rows, nheads, head_dim]: row r = x[r*x_row_stride + ...], it belongs to
 * the sequence b with cu_seqlens[b] <= r < cu_seqlens[b+1] and i is its index inside that sequence (batch strides are unused,
 * seqlen = max_seqlen is informative; rows behind cu_seqlens[batch] belong to no sequence and are left unrotated).
 * Position of row i of batch b: i + seqlen_offset + (seqlen_offsets ? seqlen_offsets[b] : 0).  A position < 0 or >= seqlen_ro
 * leaves the row unrotated - copied when out != x, untouched in place - and nothing outside cos / sin is read (fa_fwd_kvcache's
 * rule).  Columns [rotary_dim, head_dim) are copied when out != x and neither read nor written when out == x.
 * out == x (the same base address AND strides) is in place and is the common case.
 * One kernel launch on `stream`: byte movement, no atomics, no workspace, no host synchronisation, bitwise repeatable.  16-byte
 * streamed loads and stores where every x / out base address and stride is a multiple of 16 bytes, rotary_dim % 16 == 0
 * (interleaved: % 8 == 0), cos / sin are of `dtype` and 16-byte aligned, and - for out != x - (head_dim - rotary_dim) % 8 == 0;
 * one pair per lane otherwise (any even rotary_dim, 2-byte aligned views, fp32 cos / sin).  Both forms give the same bits.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL x / out / cos / sin; a dtype other than FA_FP16 /
 * FA_BF16; rotary_dim odd, <= 0 or > head_dim; negative sizes, strides or seqlen_offset; x / out not 2-byte aligned; cos / sin
 * not aligned to their element size; seqlen_offsets / cu_seqlens not 4-byte aligned; an out whose address range overlaps x's
 * without out being x itself (base address and strides).  An empty problem returns FA_OK without a launch.
 */
typedef struct fa_rotary_params {
    size_t         struct_size;      /* sizeof(fa_rotary_params) as the caller compiled it */
    const void*    x;                /* [batch, seqlen, nheads, head_dim] (cu_seqlens: [total_rows, nheads, head_dim]) of `dtype` */
    void*          out;              /* same shape, own strides; may equal x */
    int64_t        x_batch_stride, x_row_stride, x_head_stride;   /* elements, the last dimension contiguous */
    int64_t        o_batch_stride, o_row_stride, o_head_stride;
    int32_t        batch, seqlen, nheads, head_dim;   /* cu_seqlens: seqlen = max_seqlen */
    int32_t        rotary_dim;       /* even, 0 < rotary_dim <= head_dim */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    const void*    cos;              /* [seqlen_ro, rotary_dim / 2] contiguous */
    const void*    sin;
    int32_t        cos_sin_fp32;     /* 0: cos / sin of `dtype`; 1: fp32 */
    int32_t        seqlen_ro;
    int32_t        interleaved;
    int32_t        conjugate;
    int32_t        seqlen_offset;    /* host scalar, >= 0 */
    int32_t        total_rows;       /* cu_seqlens: rows of the packed tensor */
    const int32_t* seqlen_offsets;   /* device [batch], or NULL */
    const int32_t* cu_seqlens;       /* device [batch + 1], or NULL (dense) */
} fa_rotary_params;

int    fa_rotary(const fa_rotary_params* r, void* stream);
size_t fa_rotary_params_size(void);

/*
 * fa_kv_store - write a ragged packed batch of K / V rows into a KV cache (additive, like the blocks above: fa_params and
 * FA_ABI_VERSION are unchanged).  The step between a ragged prefill (fa_varlen_fwd) and everything that reads a cache
 * (fa_fwd_kvcache, fa_varlen_fwd with a block_table); fa_fwd_kvcache's own append takes a uniform [B, T_new] block only.
 *
 * k, v: [total_rows, nheads, head_dim] of `dtype` (FA_FP16 / FA_BF16); element (r, h, d) of k = k[r*k_row_stride + h*k_head_stride
 * + d] (strides in elements, the last dimension contiguous) - the K and V heads of a packed [T, Hq + 2 Hk, D] qkv are such views.
 * k_cache, v_cache: [num_blocks, page_block_size, nheads, head_dim] of `cache_dtype` (= dtype, or FA_FP8_E4M3) with explicit
 * batch (page), row and head strides in elements of the cache type, K and V each their own.  A contiguous cache
 * [Bc, S_max, nheads, head_dim] is num_blocks = Bc, page_block_size = S_max, paged = 0.
 * Exactly one of two addressing modes:
 *   slot mode (slot_mapping != NULL): row r goes to block slot_mapping[r] / page_block_size, row slot_mapping[r] % page_block_size.
 *     A slot < 0 or >= num_blocks * page_block_size skips the row (padding rows of a captured graph).  cu_seqlens, cache_seqlens,
 *     block_table, cache_batch_idx and the rotary fields must be unset.
 *   sequence mode (cu_seqlens != NULL): row r belongs to the sequence b with cu_seqlens[b] <= r < cu_seqlens[b+1], has the index
 *     i = r - cu_seqlens[b] and goes to position cache_seqlens[b] + i (cache_seqlens NULL: i) - fa_fwd_kvcache's append rule for
 *     a ragged batch.  paged != 0: page block_table[b*block_table_batch_stride + pos / page_block_size], row pos % page_block_size,
 *     capacity max_blocks * page_block_size; paged == 0: batch slot cache_batch_idx[b] (NULL: b, which needs batch <= num_blocks),
 *     row pos, capacity page_block_size.  A position < 0 or >= the capacity is dropped without a write, as in the append; rows
 *     behind cu_seqlens[batch] belong to no sequence and are dropped; empty sequences are legal; a block-table entry is read only
 *     for a row that is stored (entries are not range-checked, as in fa_fwd_kvcache).
 * Two rows with the same destination: one of them wins (unspecified, as in fa_scatter_rows).
 * fp8 cache: stored code = e4m3(clamp(x * (1 / descale), -448, 448)), round to nearest even - the expression, the reciprocal and
 * the conversion are fa_fwd_kvcache's append's own (one shared header), so both write the same codes.  k_descale / v_descale: host
 * floats, 0 = 1.0; ignored for a 16-bit cache.
 * RoPE on K (sequence mode only, rotary_dim > 0): row i of sequence b is rotated at its cache position cache_seqlens[b] + i with
 * fa_fwd_kvcache's in-kernel rule and arithmetic (fp32 math, one rounding to `dtype`, then - fp8 cache - the quantisation above);
 * rotary_cos / rotary_sin: [seqlen_ro, rotary_dim / 2] of `dtype`, contiguous.  A position outside [0, seqlen_ro) stores the row
 * unrotated and reads nothing outside the tables.  V is never rotated.
 * One kernel launch on `stream` stores K and V: byte movement, no LDS, no atomics, no workspace, no host synchronisation, bitwise
 * repeatable.  16-byte loads; 16-byte stores (fp8 caches: 16-byte stores where head_dim % 16 == 0 and every cache base and stride
 * is a multiple of 16 bytes, 8-byte stores otherwise).
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL k, v, k_cache or v_cache; both addressing modes or
 * neither; block_table together with cache_batch_idx; block_table without paged, or sequence mode with paged and no block_table;
 * sequence-mode or rotary fields in slot mode; a dtype other than FA_FP16 / FA_BF16; a cache_dtype other than dtype or
 * FA_FP8_E4M3; head_dim not a multiple of 8 or above 256; negative sizes or strides; page_block_size <= 0; a contiguous cache
 * without cache_batch_idx and batch > num_blocks; k / v bases or strides that are not multiples of 16 bytes; cache bases or
 * strides that are not multiples of 16 bytes (fp8: 8 bytes); a slot_mapping that is not 8-byte aligned; int32 side arrays that
 * are not 4-byte aligned; a negative or non-finite descale; rotary_cos / rotary_sin not both given, rotary_dim > head_dim or
 * not a multiple of 16, tables not 16-byte aligned.  total_rows == 0, nheads == 0 or (sequence mode) batch == 0: FA_OK without
 * a launch.
 */
typedef struct fa_kv_store_params {
    size_t         struct_size;      /* sizeof(fa_kv_store_params) as the caller compiled it */
    const void*    k;                /* [total_rows, nheads, head_dim] of `dtype`, read only */
    const void*    v;
    int64_t        k_row_stride, k_head_stride;        /* elements, the last dimension contiguous */
    int64_t        v_row_stride, v_head_stride;
    void*          k_cache;          /* [num_blocks, page_block_size, nheads, head_dim] of `cache_dtype`, written */
    void*          v_cache;
    int64_t        kc_batch_stride, kc_row_stride, kc_head_stride;   /* elements of the cache type */
    int64_t        vc_batch_stride, vc_row_stride, vc_head_stride;
    int32_t        total_rows;       /* rows of k / v */
    int32_t        nheads;           /* KV heads */
    int32_t        head_dim;         /* a multiple of 8, <= 256 */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        cache_dtype;      /* dtype, or FA_FP8_E4M3 */
    int32_t        paged;            /* != 0: pages addressed through block_table (sequence mode); slot mode ignores it */
    int32_t        num_blocks;       /* pages, or batch slots of a contiguous cache */
    int32_t        page_block_size;  /* rows per page, or S_max of a contiguous cache; > 0 */
    const int64_t* slot_mapping;     /* slot mode: device [total_rows], 8-byte aligned */
    const int32_t* cu_seqlens;       /* sequence mode: device [batch + 1] */
    const int32_t* cache_seqlens;    /* device [batch], NULL = zeros */
    const int32_t* block_table;      /* device [batch, max_blocks], paged caches */
    int64_t        block_table_batch_stride;           /* elements */
    const int32_t* cache_batch_idx;  /* device [batch], contiguous caches; NULL = identity */
    int32_t        batch;            /* sequence mode: sequences */
    int32_t        max_blocks;       /* columns of block_table */
    float          k_descale;        /* fp8 cache: value = code * descale; 0 = 1.0 */
    float          v_descale;
    int32_t        rotary_dim;       /* 0 = no rotary; else a multiple of 16, <= head_dim */
    int32_t        rotary_interleaved;
    const void*    rotary_cos;       /* [seqlen_ro, rotary_dim / 2] of `dtype`, contiguous, 16-byte aligned */
    const void*    rotary_sin;
    int32_t        seqlen_ro;
    int32_t        reserved;         /* 0 */
} fa_kv_store_params;

int    fa_kv_store(const fa_kv_store_params* s, void* stream);
size_t fa_kv_store_params_size(void);

/*
 * fa_kv_gather - read ragged K / V rows out of a KV cache into a packed pair: fa_kv_store read backwards (additive, like the
 * blocks above: fa_params and FA_ABI_VERSION are unchanged).  What turns cache pages back into the packed tensors that the ops
 * without a block_table take (the fp8 forward, every backward, fa_merge_states' callers with a dense prefix), and the first half
 * of moving rows inside a cache: gather by slot into a staging pair, then fa_kv_store by slot.
 *
 * k_cache, v_cache: [num_blocks, page_block_size, nheads, head_dim] of `cache_dtype` (FA_FP16, FA_BF16 or FA_FP8_E4M3), read only,
 * with explicit batch (page), row and head strides in elements of the cache type, K and V each their own.  A contiguous cache
 * [Bc, S_max, nheads, head_dim] is num_blocks = Bc, page_block_size = S_max, paged = 0.
 * k, v: [total_rows, nheads, head_dim] of `dtype` (FA_FP16 / FA_BF16), written; element (r, h, d) of k = k[r*k_row_stride +
 * h*k_head_stride + d] (strides in elements, the last dimension contiguous) - the K and V heads of a packed [T, Hq + 2 Hk, D] qkv
 * are such views.  A 16-bit cache must have cache_dtype == dtype.
 * Exactly one of two addressing modes, fa_kv_store's:
 *   slot mode (slot_mapping != NULL): row r is block slot_mapping[r] / page_block_size, row slot_mapping[r] % page_block_size.
 *     cu_seqlens, seq_offsets, block_table and cache_batch_idx must be unset.
 *   sequence mode (cu_seqlens != NULL): row r belongs to the sequence b with cu_seqlens[b] <= r < cu_seqlens[b+1], has the index
 *     i = r - cu_seqlens[b] and reads position seq_offsets[b] + i (seq_offsets NULL: i) - the counterpart of the store's
 *     cache_seqlens: the first position of the run that is read.  paged != 0: page block_table[b*block_table_batch_stride + pos /
 *     page_block_size], row pos % page_block_size, capacity max_blocks * page_block_size; paged == 0: batch slot
 *     cache_batch_idx[b] (NULL: b, which needs batch <= num_blocks), row pos, capacity page_block_size.
 * EVERY output row is written exactly once.  A row that names nothing - a slot < 0 or >= num_blocks * page_block_size, a
 * position < 0 or >= the capacity, a row behind cu_seqlens[batch] - is written as zeros (+0 bits) in k and v: the padding-row
 * rule of a captured graph turned round, the whole output is defined.  Empty sequences are legal; a block-table entry is read
 * only for a row that is gathered (entries are not range-checked, as in fa_fwd_kvcache).
 * 16-bit cache: copied bit for bit (NaN payloads, -0).  fp8 cache: out = round_to_nearest_even_to_dtype(fp32(code) * descale) -
 * the exact conversion of the code, one fp32 multiply, one rounding; torch: (cache.float() * descale).to(dtype).  k_descale /
 * v_descale: host floats, 0 = 1.0; ignored for a 16-bit cache.
 * One kernel launch on `stream` reads K and V: byte movement, no LDS, no atomics, no workspace, no host synchronisation, bitwise
 * repeatable.  16-byte stores; 16-byte loads (fp8 caches: 16-byte loads where head_dim % 16 == 0 and every cache base and stride
 * is a multiple of 16 bytes, 8-byte loads otherwise - the same bits either way).
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL k, v, k_cache or v_cache; both addressing modes or
 * neither; block_table together with cache_batch_idx; block_table without paged, or sequence mode with paged and no block_table;
 * sequence-mode fields in slot mode; a dtype other than FA_FP16 / FA_BF16; a cache_dtype other than dtype or FA_FP8_E4M3;
 * head_dim not a multiple of 8 or above 256; negative sizes or strides; page_block_size <= 0; a contiguous cache without
 * cache_batch_idx and batch > num_blocks; k / v bases or strides that are not multiples of 16 bytes; cache bases or strides that
 * are not multiples of 16 bytes (fp8: 8 bytes); a slot_mapping that is not 8-byte aligned; int32 side arrays that are not 4-byte
 * aligned; a negative or non-finite descale; k or v whose address range overlaps k_cache's or v_cache's.  total_rows == 0 or
 * nheads == 0: FA_OK without a launch; sequence mode with batch == 0 and total_rows > 0 zero-fills the rows.
 */
typedef struct fa_kv_gather_params {
    size_t         struct_size;      /* sizeof(fa_kv_gather_params) as the caller compiled it */
    const void*    k_cache;          /* [num_blocks, page_block_size, nheads, head_dim] of `cache_dtype`, read only */
    const void*    v_cache;
    int64_t        kc_batch_stride, kc_row_stride, kc_head_stride;   /* elements of the cache type */
    int64_t        vc_batch_stride, vc_row_stride, vc_head_stride;
    void*          k;                /* [total_rows, nheads, head_dim] of `dtype`, written */
    void*          v;
    int64_t        k_row_stride, k_head_stride;        /* elements, the last dimension contiguous */
    int64_t        v_row_stride, v_head_stride;
    int32_t        total_rows;       /* rows of k / v */
    int32_t        nheads;           /* KV heads */
    int32_t        head_dim;         /* a multiple of 8, <= 256 */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        cache_dtype;      /* dtype, or FA_FP8_E4M3 */
    int32_t        paged;            /* != 0: pages addressed through block_table (sequence mode); slot mode ignores it */
    int32_t        num_blocks;       /* pages, or batch slots of a contiguous cache */
    int32_t        page_block_size;  /* rows per page, or S_max of a contiguous cache; > 0 */
    const int64_t* slot_mapping;     /* slot mode: device [total_rows], 8-byte aligned */
    const int32_t* cu_seqlens;       /* sequence mode: device [batch + 1] */
    const int32_t* seq_offsets;      /* device [batch]: first position read of each sequence, NULL = zeros */
    const int32_t* block_table;      /* device [batch, max_blocks], paged caches */
    int64_t        block_table_batch_stride;           /* elements */
    const int32_t* cache_batch_idx;  /* device [batch], contiguous caches; NULL = identity */
    int32_t        batch;            /* sequence mode: sequences */
    int32_t        max_blocks;       /* columns of block_table */
    float          k_descale;        /* fp8 cache: value = code * descale; 0 = 1.0 */
    float          v_descale;
} fa_kv_gather_params;

int    fa_kv_gather(const fa_kv_gather_params* s, void* stream);
size_t fa_kv_gather_params_size(void);

/*
 * fa_rope_store - the prologue of a serving step in one launch: rotate q and k at PER-TOKEN positions and store K / V into the KV
 * cache by slot (additive, like the blocks above: fa_params and FA_ABI_VERSION are unchanged).  What fa_rotary (positions = row
 * index + a per-sequence offset) followed by fa_kv_store in slot mode (no rotation) do in two or three launches, for a flat token
 * batch with positions[T] and slot_mapping[T] - draft-tree nodes, re-packed tokens and padding rows included.
 *
 * q: [total_rows, nheads_q, head_dim] of `dtype` (FA_FP16 / FA_BF16), or NULL (a K / V-only call); k, v: [total_rows, nheads_k,
 * head_dim]; element (r, h, d) of q = q[r*q_row_stride + h*q_head_stride + d] (strides in elements, the last dimension contiguous)
 * - the q, k and v heads of one packed [T, Hq + 2 Hk, D] qkv are such views.  q_out, k_out: the same shapes with their own strides.
 * q_out == q (the same base address AND strides) is in place, likewise k_out == k; k_out == NULL: the rotated K is not written
 * back, only cached; q_out is required whenever q is given.  The caller guarantees that the q, k and v views share no element.
 * positions: device int64 [total_rows].  pos = positions[r]; row r of q and of k is rotated if and only if 0 <= pos < seqlen_ro,
 * with fa_rotary's pair rule and arithmetic (fp32 math, c = cos[pos, t], s = sin[pos, t], one rounding to `dtype`;
 * rotary_interleaved != 0: pairs (2t, 2t+1), otherwise (t, t + rotary_dim/2)).  Any other position leaves the row unrotated -
 * copied when out != in, untouched in place - and nothing outside rotary_cos / rotary_sin ([seqlen_ro, rotary_dim / 2] of `dtype`,
 * contiguous) is read.  Columns [rotary_dim, head_dim) are copied when out != in and neither read nor written in place.
 * q_out[r] and k_out[r] are written for EVERY row, whatever its slot: their bits are fa_rotary's.
 * k_cache, v_cache, their strides, num_blocks, page_block_size, cache_dtype, k_descale, v_descale and slot_mapping are fa_kv_store's
 * slot mode: s = slot_mapping[r]; s < 0 or s >= num_blocks * page_block_size skips the cache write of that row (padding rows of a
 * captured graph); otherwise block s / page_block_size, row s % page_block_size gets k_cache = store(rope(k[r], pos)) and
 * v_cache = store(v[r]), where store is a bit copy for a 16-bit cache and fa_kv_store's e4m3(clamp(x * (1 / descale), -448, 448))
 * for an fp8 cache: the cache holds the bits that fa_rotary followed by fa_kv_store by slot would leave.  V is never rotated.  Two
 * rows with the same slot: one of them wins (unspecified, as in fa_kv_store).
 * k_cache == v_cache == NULL is the rotate-only form: v and slot_mapping must be NULL too and at least one of q / k_out must be
 * given - the standalone rotation at per-token positions.
 * One kernel launch on `stream`: byte movement, no LDS, no atomics, no workspace, no host synchronisation, bitwise repeatable,
 * capturable in a graph.  One lane owns both partner pieces of a GPT-NeoX pair and loads everything it owns before its first
 * store, so in place no element is read after its partner was written.  16-byte loads; 16-byte stores to q_out / k_out and to
 * 16-bit caches; fp8 caches: 16-byte stores where head_dim % 16 == 0, every cache base and stride is a multiple of 16 bytes and
 * (GPT-NeoX pairs only) rotary_dim % 32 == 0, 8-byte stores otherwise - the same bits either way.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL k, positions, rotary_cos or rotary_sin; q without q_out
 * or q_out without q; exactly one of the two caches; caches without v or without slot_mapping; v or slot_mapping without caches;
 * the rotate-only form with neither q nor k_out; a dtype other than FA_FP16 / FA_BF16; a cache_dtype other than dtype or
 * FA_FP8_E4M3; head_dim not a multiple of 8 or above 256; rotary_dim <= 0, not a multiple of 16 or > head_dim; negative sizes or
 * strides; page_block_size <= 0 with caches; q / k / v / q_out / k_out bases or strides that are not multiples of 16 bytes; cache
 * bases or strides that are not multiples of 16 bytes (fp8: 8 bytes); positions or slot_mapping not 8-byte aligned; rotary_cos /
 * rotary_sin not 16-byte aligned; a negative or non-finite descale; a q_out / k_out that shares its input's base address but not
 * its strides; an out-of-place q_out or k_out whose address range overlaps that of q, k, v, positions, slot_mapping, rotary_cos,
 * rotary_sin, k_cache or v_cache.  total_rows == 0 or nheads_q == nheads_k == 0 (a NULL q counts as no q heads): FA_OK without a
 * launch.
 */
typedef struct fa_rope_store_params {
    size_t         struct_size;      /* sizeof(fa_rope_store_params) as the caller compiled it */
    const void*    q;                /* [total_rows, nheads_q, head_dim] of `dtype`, or NULL */
    const void*    k;                /* [total_rows, nheads_k, head_dim] */
    const void*    v;                /* [total_rows, nheads_k, head_dim]; NULL in the rotate-only form */
    int64_t        q_row_stride, q_head_stride;        /* elements, the last dimension contiguous */
    int64_t        k_row_stride, k_head_stride;
    int64_t        v_row_stride, v_head_stride;
    void*          q_out;            /* q's shape, own strides; may equal q; required with q */
    void*          k_out;            /* k's shape, own strides; may equal k; NULL: the rotated K is only cached */
    int64_t        qo_row_stride, qo_head_stride;
    int64_t        ko_row_stride, ko_head_stride;
    const int64_t* positions;        /* device [total_rows], 8-byte aligned */
    const void*    rotary_cos;       /* [seqlen_ro, rotary_dim / 2] of `dtype`, contiguous, 16-byte aligned */
    const void*    rotary_sin;
    int32_t        rotary_dim;       /* a multiple of 16, 0 < rotary_dim <= head_dim */
    int32_t        seqlen_ro;
    int32_t        rotary_interleaved;
    int32_t        total_rows;       /* rows of q / k / v */
    int32_t        nheads_q;
    int32_t        nheads_k;
    int32_t        head_dim;         /* a multiple of 8, <= 256 */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        cache_dtype;      /* dtype, or FA_FP8_E4M3; read with caches only */
    int32_t        reserved;         /* 0 */
    void*          k_cache;          /* [num_blocks, page_block_size, nheads_k, head_dim] of `cache_dtype`, written; or NULL */
    void*          v_cache;
    int64_t        kc_batch_stride, kc_row_stride, kc_head_stride;   /* elements of the cache type */
    int64_t        vc_batch_stride, vc_row_stride, vc_head_stride;
    int32_t        num_blocks;       /* pages, or batch slots of a contiguous cache */
    int32_t        page_block_size;  /* rows per page, or S_max of a contiguous cache; > 0 with caches */
    const int64_t* slot_mapping;     /* device [total_rows], 8-byte aligned; with caches */
    float          k_descale;        /* fp8 cache: value = code * descale; 0 = 1.0 */
    float          v_descale;
} fa_rope_store_params;

int    fa_rope_store(const fa_rope_store_params* s, void* stream);
size_t fa_rope_store_params_size(void);

/*
 * fa_qk_norm_rope_store - fa_rope_store with a per-head RMSNorm of q and k in front of the rotation, still one launch (additive,
 * like the blocks above: fa_params and FA_ABI_VERSION are unchanged).  The prologue of a serving step for models with QK-norm
 * (Qwen3, Gemma 3, OLMo 2): norm over head_dim with a learned [head_dim] weight, rotation at per-token positions, K / V store.
 *
 * The block is fa_rope_store_params field for field (same order, same meaning, same rules) followed by the norm's fields.  For
 * every row r and every head h of q (weight q_weight) and of k (weight k_weight):
 *     ss   = sum_d x[r,h,d]^2                                         fp32
 *     rstd = 1 / sqrt(ss / head_dim + eps)                            fp32
 *     y[d] = round_to_dtype((x[d] * rstd) * (weight_offset + w[d]))   fp32 products, ONE rounding to `dtype`
 * and that 16-bit y is what fa_rope_store's rotation, write-back and cache store then see: the call leaves the bits of "norm-only
 * call, then fa_rope_store".  The sum has a fixed order (csrc/fa_rmsnorm.h): a head's bits do not depend on what else is in the
 * batch.  A row whose position is outside [0, seqlen_ro) is normalised and left unrotated; a row whose slot is outside the cache
 * is normalised and rotated, only its cache write is skipped.  V is neither normalised nor rotated.
 * q_weight, k_weight: device [head_dim] of `weight_dtype` (FA_FP16 / FA_BF16 - then it must equal `dtype` - or FA_FP32),
 * contiguous, 16-byte aligned.  Either may be NULL: that tensor is not normalised, only rotated; with both NULL the call leaves
 * fa_rope_store's bits.  In place (q_out == q, k_out == k) a normalised tensor is rewritten in every column, a tensor without a
 * weight as in fa_rope_store.  weight_offset: Gemma's (1 + w) is 1.0.
 * seqlen_ro == 0 is the form without rotation: rotary_dim, rotary_interleaved, positions, rotary_cos and rotary_sin are ignored
 * (and may be 0 / NULL) - norm only without caches, norm + store with them.
 * One kernel launch on `stream`: no LDS, no atomics, no workspace, no host synchronisation, bitwise repeatable, capturable in a
 * graph.  A head is owned by adjacent lanes of one wave, 8 columns each; the row sum and the GPT-NeoX partner piece travel between
 * lanes, so in place a lane only ever loads its own columns, and it loads them before its first store.  16-byte loads and
 * stores, 8-byte stores to fp8 caches.
 * FA_ERR_INVALID_ARGUMENT before any launch: everything fa_rope_store lists (a NULL positions / rotary_cos / rotary_sin and a bad
 * rotary_dim only where seqlen_ro > 0); a weight_dtype other than `dtype` or FA_FP32 where a weight is given; a weight that is not
 * 16-byte aligned; a negative or non-finite eps; a non-finite weight_offset; an out-of-place q_out or k_out that overlaps a
 * weight.  total_rows == 0 or nheads_q == nheads_k == 0 (a NULL q counts as no q heads): FA_OK without a launch.
 */
typedef struct fa_qk_norm_rope_store_params {
    size_t         struct_size;      /* sizeof(fa_qk_norm_rope_store_params) as the caller compiled it */
    const void*    q;                /* from here to v_descale: fa_rope_store_params */
    const void*    k;
    const void*    v;
    int64_t        q_row_stride, q_head_stride;
    int64_t        k_row_stride, k_head_stride;
    int64_t        v_row_stride, v_head_stride;
    void*          q_out;
    void*          k_out;
    int64_t        qo_row_stride, qo_head_stride;
    int64_t        ko_row_stride, ko_head_stride;
    const int64_t* positions;        /* may be NULL where seqlen_ro == 0 */
    const void*    rotary_cos;       /* may be NULL where seqlen_ro == 0 */
    const void*    rotary_sin;
    int32_t        rotary_dim;
    int32_t        seqlen_ro;        /* 0: no rotation */
    int32_t        rotary_interleaved;
    int32_t        total_rows;
    int32_t        nheads_q;
    int32_t        nheads_k;
    int32_t        head_dim;
    int32_t        dtype;
    int32_t        cache_dtype;
    int32_t        reserved;         /* 0 */
    void*          k_cache;
    void*          v_cache;
    int64_t        kc_batch_stride, kc_row_stride, kc_head_stride;
    int64_t        vc_batch_stride, vc_row_stride, vc_head_stride;
    int32_t        num_blocks;
    int32_t        page_block_size;
    const int64_t* slot_mapping;
    float          k_descale;
    float          v_descale;
    const void*    q_weight;         /* device [head_dim] of `weight_dtype`, 16-byte aligned; NULL: q is not normalised */
    const void*    k_weight;         /* NULL: k is not normalised */
    int32_t        weight_dtype;     /* `dtype`, or FA_FP32; read where a weight is given */
    float          eps;              /* >= 0, finite */
    float          weight_offset;    /* y = x rstd (weight_offset + w) */
    int32_t        reserved1;        /* 0 */
} fa_qk_norm_rope_store_params;

int    fa_qk_norm_rope_store(const fa_qk_norm_rope_store_params* s, void* stream);
size_t fa_qk_norm_rope_store_params_size(void);

/*
 * fa_qk_norm_rope_bwd - the backward of fa_qk_norm_rope_store's norm + rotation (additive: fa_params and FA_ABI_VERSION are
 * unchanged).  The forward computes, for every row r and every head of q (weight q_weight) and of k (k_weight),
 *     y = round_to_dtype(x * rstd * g),  g = weight_offset + w,  rstd = 1 / sqrt(mean_d(x^2) + eps),   z = rope(y) at positions[r]
 * (z = y where the position is outside [0, seqlen_ro), in columns >= rotary_dim, or where seqlen_ro == 0).  From dz - dq_out /
 * dk_out, the gradients of q_out / k_out - and the saved PRE-NORM inputs q / k this op computes, with BOTH 16-bit roundings of the
 * forward treated as the identity (straight-through) and all arithmetic in fp32:
 *     dy = conj_rope(dz)        fa_rotary's pair rule with the sign of sin flipped exactly, NOT rounded; dy = dz where the forward
 *                               left the element unrotated
 *   a tensor WITHOUT a weight:  dx = round_to_dtype(dy)       - the bits of fa_rotary with `conjugate` at the same positions
 *   a tensor WITH a weight:     xhat = x * rstd;  a = dy * g;  c = (sum_d a[d] xhat[d]) / head_dim
 *                               dx    = round_to_dtype(rstd * (a - xhat * c))      (a - xhat c is one fused multiply-add)
 *                               dw[d] = sum over ALL rows and all heads of that tensor of dy[d] * xhat[d]
 * rstd is recomputed from x with the forward's fixed-order sum (csrc/fa_rmsnorm.h): it has the forward's bits, the forward saves
 * nothing.  The sum for c has the same fixed order, so a head's dx bits do not depend on what else is in the batch.  Every row
 * enters dw, rows whose position is outside the tables included: there is no notion of a padding row.  eps == 0 with an all-zero
 * head gives what the arithmetic gives (non-finite values), as in the forward.
 * dq_out, dk_out, q, k, dq, dk: [total_rows, nheads, head_dim] of `dtype`, each with its own row and head stride (elements, the
 * last dimension contiguous) - the heads of a packed [T, Hq + 2 Hk, D] gradient are such views.  dq == dq_out and dk == dk_out
 * (the same base address AND strides) are in place and the only legal overlap.  positions, rotary_cos, rotary_sin, rotary_dim,
 * seqlen_ro (0: no rotation; the pointers may then be NULL), rotary_interleaved, q_weight, k_weight, weight_dtype, eps and
 * weight_offset are fa_qk_norm_rope_store's.  dq_weight, dk_weight: device [head_dim] of `weight_dtype`, 16-byte aligned, written
 * ONCE with one rounding of the final fp32 sum.
 * Any of the four outputs dq, dk, dq_weight, dk_weight may be NULL and is then skipped; a tensor of which nothing is wanted is not
 * read.  A NULL q counts as no q heads (dq_out, dq may then be NULL as well).  k and dk_out are required.
 * dw is deterministic, no atomics: a lane keeps its partial sums in registers over the rows it walks, a workgroup adds its lanes
 * through LDS in a fixed order and writes one fp32 row [2][head_dim] into `workspace`, and a second small kernel on the same
 * stream adds the rows in a fixed order.  The grid and with it the order depend on this block alone, never on the device:
 * fa_qk_norm_rope_bwd_workspace_bytes() needs no device and the bits are the same on every card.  The workspace is 0 bytes where
 * neither dq_weight nor dk_weight is given (then: one launch, no LDS); otherwise it must be 16-byte aligned and hold the reported
 * size (at most 2 MB).
 * No host synchronisation, bitwise repeatable, capturable in a graph.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL k or dk_out; q without dq_out; dq without q; dq_weight
 * without q_weight or dk_weight without k_weight; non-zero reserved fields; NULL positions / rotary_cos / rotary_sin or a
 * rotary_dim that is not a positive multiple of 16 <= head_dim where seqlen_ro > 0; a dtype other than FA_FP16 / FA_BF16; a
 * weight_dtype other than `dtype` or FA_FP32 where a weight is given; head_dim not a multiple of 8 or above 256; negative sizes
 * or strides; tensor bases or strides, weights, weight gradients, tables or the workspace not 16-byte aligned; positions not
 * 8-byte aligned; a negative or non-finite eps; a non-finite weight_offset; a dq / dk that shares its gradient's base address but
 * not its strides; an output (dq, dk, dq_weight, dk_weight) whose address range overlaps an input other than by that exact
 * aliasing, another output or the workspace; a workspace that overlaps an input; a workspace smaller than reported.
 * total_rows == 0, or no heads (nheads_k == 0 and no q heads): FA_OK without a kernel launch; a dq_weight / dk_weight that was
 * asked for is then set to zeros on `stream`.
 */
typedef struct fa_qk_norm_rope_bwd_params {
    size_t         struct_size;      /* sizeof(fa_qk_norm_rope_bwd_params) as the caller compiled it */
    const void*    dq_out;           /* [total_rows, nheads_q, head_dim] of `dtype`: the gradient of q_out; NULL with a NULL q */
    const void*    dk_out;           /* [total_rows, nheads_k, head_dim]: the gradient of k_out */
    int64_t        dqo_row_stride, dqo_head_stride;    /* elements, the last dimension contiguous */
    int64_t        dko_row_stride, dko_head_stride;
    const void*    q;                /* the forward's pre-norm q, or NULL: no q heads */
    const void*    k;                /* the forward's pre-norm k */
    int64_t        q_row_stride, q_head_stride;
    int64_t        k_row_stride, k_head_stride;
    void*          dq;               /* q's shape, own strides; may equal dq_out; NULL: skipped */
    void*          dk;               /* k's shape, own strides; may equal dk_out; NULL: skipped */
    int64_t        dq_row_stride, dq_head_stride;
    int64_t        dk_row_stride, dk_head_stride;
    const int64_t* positions;        /* device [total_rows], 8-byte aligned; may be NULL where seqlen_ro == 0 */
    const void*    rotary_cos;       /* [seqlen_ro, rotary_dim / 2] of `dtype`, contiguous, 16-byte aligned */
    const void*    rotary_sin;
    int32_t        rotary_dim;       /* a multiple of 16, 0 < rotary_dim <= head_dim (read where seqlen_ro > 0) */
    int32_t        seqlen_ro;        /* 0: no rotation */
    int32_t        rotary_interleaved;
    int32_t        total_rows;
    int32_t        nheads_q;
    int32_t        nheads_k;
    int32_t        head_dim;         /* a multiple of 8, <= 256 */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    const void*    q_weight;         /* device [head_dim] of `weight_dtype`, 16-byte aligned; NULL: q was not normalised */
    const void*    k_weight;         /* NULL: k was not normalised */
    int32_t        weight_dtype;     /* `dtype`, or FA_FP32; read where a weight is given */
    float          eps;              /* >= 0, finite: the forward's */
    float          weight_offset;    /* the forward's */
    int32_t        reserved;         /* 0 */
    void*          dq_weight;        /* device [head_dim] of `weight_dtype`, 16-byte aligned; NULL: skipped */
    void*          dk_weight;
    void*          workspace;        /* fa_qk_norm_rope_bwd_workspace_bytes() bytes, 16-byte aligned; may be NULL where that is 0 */
    size_t         workspace_bytes;
    int64_t        reserved1[2];     /* 0 */
} fa_qk_norm_rope_bwd_params;

int    fa_qk_norm_rope_bwd(const fa_qk_norm_rope_bwd_params* s, void* stream);
/* the workspace of that call; `workspace`, `workspace_bytes` and where the tensors lie are not looked at (the overlap rules are the
 * call's); 0 for a block that the call rejects for any other reason */
size_t fa_qk_norm_rope_bwd_workspace_bytes(const fa_qk_norm_rope_bwd_params* s);
size_t fa_qk_norm_rope_bwd_params_size(void);

/*
 * fa_add_norm - residual add + RMSNorm / LayerNorm over the whole hidden size, one launch (additive: fa_params and FA_ABI_VERSION
 * are unchanged).  x: [rows, n] of `dtype` (fp16 / bf16).  All arithmetic is fp32:
 *     z            = x                                                (residual NULL)
 *     z            = round_res(float(x) + float(residual))           ONE fp32 add, ONE rounding to residual_out_dtype
 *     residual_out = z                                                (required with a residual; without one it is optional
 *                                                                      and gets float(x) or x: the prenorm copy)
 *     RMSNorm:   rstd = 1 / sqrt(sum(z^2) / n + eps);                     xhat = z * rstd
 *     LayerNorm: mean = sum(z) / n;  rstd = 1 / sqrt(sum((z - mean)^2) / n + eps);  xhat = (z - mean) * rstd   (two passes)
 *     out = round_to_dtype(xhat * g)           g = weight_offset + weight   (weight_offset 1.0: Gemma, zero-centred weights)
 *     out = round_to_dtype(fma(xhat, g, b))    with a bias b (one fused multiply-add)
 * The norm reads the STORED z - the value residual_out holds -, so fa_add_norm(x, residual) leaves in `out` exactly the bits of
 * fa_add_norm(residual_out) when residual_out_dtype == dtype, as the HF modules and vLLM's fused_add_rms_norm do; a backward can
 * recompute mean / rstd from residual_out and the forward saves nothing.
 * The order of every row sum is fixed and depends on n alone (csrc/fa_rowsum.h): a row's bits do not depend on the number of rows,
 * on the row's index or on the device.  n <= 256: the row is owned by G adjacent lanes of a wave as a head is in
 * fa_qk_norm_rope_store (csrc/fa_rmsnorm.h), and an RMSNorm without bias has that op's bits for a head of n columns.
 * x, residual, out, residual_out: each with its own row stride in elements (a multiple of 8), the last dimension contiguous,
 * 16-byte aligned bases.  residual_dtype: `dtype` or FA_FP32.  residual_out_dtype: `dtype` or FA_FP32; FA_FP32 where
 * residual_dtype is FA_FP32.  weight, bias: device [n] of `weight_dtype` (`dtype` or FA_FP32), 16-byte aligned; bias may be NULL.
 * In place: out == x (the same base address AND row stride), and residual_out == residual (base, row stride and dtype) are
 * legal - a lane loads everything it owns before its first store.  Every other overlap of an output with an input or with the
 * other output is rejected.
 * No workspace, no atomics, no host synchronisation, bitwise repeatable, capturable in a graph.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL x, out or weight; a residual without residual_out; a
 * dtype other than FA_FP16 / FA_BF16; a residual_dtype / residual_out_dtype / weight_dtype other than `dtype` or FA_FP32, or a
 * 16-bit residual_out_dtype with an fp32 residual; n not a multiple of 8 or outside [8, 16384]; negative rows or row strides; a
 * row stride that is not a multiple of 8 elements or (rows > 1) smaller than n; bases, weight or bias not 16-byte aligned; a
 * negative or non-finite eps; a non-finite weight_offset; an illegal overlap; non-zero reserved fields.  rows > 2^31 - 1:
 * FA_ERR_UNSUPPORTED.  rows == 0: FA_OK without a launch.
 */
typedef struct fa_add_norm_params {
    size_t         struct_size;      /* sizeof(fa_add_norm_params) as the caller compiled it */
    const void*    x;                /* [rows, n] of `dtype` */
    const void*    residual;         /* [rows, n] of `residual_dtype`, or NULL */
    void*          out;              /* [rows, n] of `dtype`; may equal x */
    void*          residual_out;     /* [rows, n] of `residual_out_dtype`; may equal residual; NULL without a residual: not written */
    int64_t        x_row_stride, residual_row_stride, out_row_stride, residual_out_row_stride;     /* elements */
    const void*    weight;           /* device [n] of `weight_dtype`, 16-byte aligned */
    const void*    bias;             /* device [n] of `weight_dtype`, or NULL */
    int64_t        rows;
    int32_t        n;                /* a multiple of 8, 8 .. 16384 */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        residual_dtype;   /* `dtype` or FA_FP32 (read where residual is given) */
    int32_t        residual_out_dtype;   /* `dtype` or FA_FP32 (read where residual or residual_out is given) */
    int32_t        weight_dtype;     /* `dtype` or FA_FP32 */
    int32_t        is_rms_norm;      /* 0: LayerNorm */
    float          eps;              /* >= 0, finite */
    float          weight_offset;    /* finite */
    int64_t        reserved[2];      /* 0 */
} fa_add_norm_params;

int    fa_add_norm(const fa_add_norm_params* s, void* stream);
size_t fa_add_norm_params_size(void);

/*
 * fa_add_norm_bwd - the backward of fa_add_norm.  Both roundings of the forward (z to residual_out_dtype, out to `dtype`) are
 * treated as the identity (straight-through), all arithmetic is fp32.  From dy [rows, n] of `dtype` (the gradient of out), the
 * saved z [rows, n] of `z_dtype` (residual_out; x itself where the forward had no residual), an optional dres_out [rows, n] of
 * `z_dtype` (the gradient of residual_out under prenorm) and the weight:
 *     mean, rstd: recomputed from z with the forward's fixed-order sums (csrc/fa_rowsum.h) - the forward's bits
 *     a = dy * g,  g = weight_offset + weight;   xhat = z * rstd   (LayerNorm: (z - mean) * rstd)
 *     RMSNorm:   c  = (sum_d a xhat) / n;                       dz = rstd * fma(-xhat, c, a)
 *     LayerNorm: c1 = (sum_d a) / n;  c2 = (sum_d a xhat) / n;  dz = rstd * fma(-xhat, c2, a - c1)
 *     with dres_out:  dz = fma(rstd, that fma, float(dres_out))
 *     dx   = round_to_dtype(dz)                [rows, n] of `dtype`; may equal dy (base AND row stride: in place)
 *     dres = round(dz) to `dres_dtype`         [rows, n]: the gradient of the forward's residual
 *     dweight[d] = sum over rows of dy[d] xhat[d];   dbias[d] = sum over rows of dy[d]       [n] of `weight_dtype`, one rounding
 * The sums for c, c1, c2 have the forward's fixed order: a row's dx / dres bits do not depend on what else is in the batch.  For
 * n <= 256 an RMSNorm's dx has the bits of fa_qk_norm_rope_bwd without rotation on a head of n columns.
 * Each of dx, dres, dweight, dbias may be NULL and is then skipped (with all four NULL: FA_OK, nothing is read).
 * dweight / dbias are deterministic, no atomics: a workgroup walks a run of consecutive rows with its partial sums in registers
 * (fmaf in row order), writes ONE fp32 partial row [1 or 2][n] (2 with dbias) into `workspace`, and a second small kernel on the
 * same stream adds the P partial rows - 16 contiguous runs of them in row order side by side, then the runs in order.  P <= 256
 * and the run length depend on (rows, n, dbias given) alone, never on the device: fa_add_norm_bwd_workspace_bytes() needs no
 * device, the bits are the same on every card, and the workspace is at most 256 x 2 x 16384 x 4 bytes = 32 MiB.  Without dweight
 * and dbias: one launch, a workgroup (n > 256) or a group of lanes (n <= 256) per row, no workspace.
 * No host synchronisation, bitwise repeatable, capturable in a graph.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL dy, z or weight; a dtype other than FA_FP16 / FA_BF16; a
 * z_dtype / dres_dtype / weight_dtype other than `dtype` or FA_FP32; n not a multiple of 8 or outside [8, 16384]; negative rows
 * or row strides; a row stride that is not a multiple of 8 elements or (rows > 1) smaller than n; bases, weight, dweight, dbias
 * or the workspace not 16-byte aligned; a negative or non-finite eps; a non-finite weight_offset; a dx that shares dy's base but
 * not its row stride; an output (dx, dres, dweight, dbias, the workspace) that overlaps an input other than by that aliasing, or
 * another output; a workspace smaller than reported; non-zero reserved fields.  rows > 2^31 - 1: FA_ERR_UNSUPPORTED.
 * rows == 0: FA_OK without a kernel launch; a dweight / dbias that was asked for is set to zeros on `stream`.
 */
typedef struct fa_add_norm_bwd_params {
    size_t         struct_size;      /* sizeof(fa_add_norm_bwd_params) as the caller compiled it */
    const void*    dy;               /* [rows, n] of `dtype`: the gradient of out */
    const void*    z;                /* [rows, n] of `z_dtype`: the forward's residual_out (x without a residual) */
    const void*    dres_out;         /* [rows, n] of `z_dtype`: the gradient of residual_out, or NULL */
    void*          dx;               /* [rows, n] of `dtype`; may equal dy; NULL: skipped */
    void*          dres;             /* [rows, n] of `dres_dtype`; NULL: skipped */
    int64_t        dy_row_stride, z_row_stride, dres_out_row_stride, dx_row_stride, dres_row_stride;   /* elements */
    const void*    weight;           /* device [n] of `weight_dtype`, 16-byte aligned */
    void*          dweight;          /* device [n] of `weight_dtype`, 16-byte aligned; NULL: skipped */
    void*          dbias;            /* device [n] of `weight_dtype`, 16-byte aligned; NULL: skipped */
    void*          workspace;        /* fa_add_norm_bwd_workspace_bytes() bytes, 16-byte aligned; may be NULL where that is 0 */
    size_t         workspace_bytes;
    int64_t        rows;
    int32_t        n;                /* a multiple of 8, 8 .. 16384 */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        z_dtype;          /* `dtype` or FA_FP32 */
    int32_t        dres_dtype;       /* `dtype` or FA_FP32 (read where dres is given) */
    int32_t        weight_dtype;     /* `dtype` or FA_FP32 */
    int32_t        is_rms_norm;      /* 0: LayerNorm */
    float          eps;              /* the forward's */
    float          weight_offset;    /* the forward's */
    int64_t        reserved[2];      /* 0 */
} fa_add_norm_bwd_params;

int    fa_add_norm_bwd(const fa_add_norm_bwd_params* s, void* stream);
/* the workspace of that call; `workspace`, `workspace_bytes` and where the tensors lie are not looked at; 0 for a block that the
 * call rejects for any other reason */
size_t fa_add_norm_bwd_workspace_bytes(const fa_add_norm_bwd_params* s);
size_t fa_add_norm_bwd_params_size(void);

/*
 * fa_cross_entropy - softmax cross-entropy loss over the vocabulary, forward (additive: fa_params and FA_ABI_VERSION are
 * unchanged).  logits: [rows, vocab] of `dtype` (FA_FP16, FA_BF16 or FA_FP32), last dimension contiguous, any row stride >= vocab
 * (elements); labels: int64 [rows].  All arithmetic is fp32, in this order:
 *     l_j  = logit_scale * float(logits_j)                          ONE rounding
 *     lse  = m + log(s),  m = max_j l_j,  s = sum_j exp(l_j - m)    (a running maximum and sum in a fixed order, below)
 *     loss = fma(-(1 - label_smoothing), l_label, lse)              label_smoothing == 0: lse - l_label
 *     loss = fma(-(label_smoothing / vocab), sum_j l_j, loss)       label_smoothing > 0 only; sum_j l_j is not formed otherwise
 *     z    = (lse_square_scale * lse) * lse;   loss = loss + z
 * 1 - label_smoothing and label_smoothing / vocab are fp32 operations on the host.  losses, z_losses, lse: fp32 [rows], written.
 * label == ignore_index: loss = z = +0 (lse is still written).  A label outside [0, vocab) that is not ignore_index: loss = z =
 * NaN - no address is formed from it.  A logit of -inf (a masked vocabulary entry) contributes exactly 0 to s and to sum_j l_j.
 * A row without a finite maximum - all -inf, or one that holds +inf - and a row with a NaN have lse = NaN.
 * Order: pieces are 8 columns counted from column 0 of the row; a row is cut into nchunks = ceil(vocab / CHUNK) chunks, CHUNK a
 * function of `dtype` alone; 256 lanes own the pieces of a chunk round robin and fold them in ascending order, then the lanes, the
 * waves and the chunks are merged in index order (csrc/fa_lse.h).  A row's bits depend on (vocab, dtype) and its values alone -
 * never on rows, the row's index, its alignment (a row that does not start on a 16-byte boundary is read element by element: the
 * same values) or the device.  No column >= vocab is read.
 * nchunks > 1: rows x nchunks workgroups write one 16-byte partial each into `workspace` and a second kernel on the same stream
 * merges them; fa_cross_entropy_workspace_bytes() = rows x nchunks x 16 needs no device.  nchunks == 1: one launch, no workspace.
 * No atomics, no host synchronisation, bitwise repeatable, capturable in a graph.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL logits, labels, losses, z_losses or lse; a dtype other
 * than FA_FP16 / FA_BF16 / FA_FP32; vocab < 1; negative rows or row stride, or (rows > 1) a row stride below vocab; logits not
 * aligned to their element, labels not 8-byte and the outputs not 4-byte aligned; label_smoothing outside [0, 1); a non-finite
 * logit_scale; a negative or non-finite lse_square_scale; a workspace smaller than reported or not 16-byte aligned; an output or
 * the workspace that overlaps an input or another output; non-zero reserved fields.  rows x nchunks > 2^31 - 1:
 * FA_ERR_UNSUPPORTED.  rows == 0: FA_OK without a launch.
 */
typedef struct fa_cross_entropy_params {
    size_t         struct_size;      /* sizeof(fa_cross_entropy_params) as the caller compiled it */
    const void*    logits;           /* [rows, vocab] of `dtype` */
    const int64_t* labels;           /* device [rows] */
    float*         losses;           /* device [rows] */
    float*         z_losses;         /* device [rows] */
    float*         lse;              /* device [rows]: what the backward needs, and nothing else */
    void*          workspace;        /* fa_cross_entropy_workspace_bytes() bytes, 16-byte aligned; may be NULL where that is 0 */
    size_t         workspace_bytes;
    int64_t        logits_row_stride;    /* elements */
    int64_t        rows;
    int64_t        ignore_index;     /* upstream's default: -100 */
    int32_t        vocab;            /* >= 1 */
    int32_t        dtype;            /* FA_FP16, FA_BF16 or FA_FP32 */
    float          label_smoothing;  /* [0, 1) */
    float          logit_scale;      /* finite */
    float          lse_square_scale; /* >= 0, finite: the z-loss weight */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 (room for a vocabulary-parallel form: class_start, total_classes, a precomputed lse) */
} fa_cross_entropy_params;

int    fa_cross_entropy(const fa_cross_entropy_params* s, void* stream);
/* the workspace of that call: a function of (rows, vocab, dtype); `workspace`, `workspace_bytes` and where the tensors lie are not
 * looked at; 0 for a block that the call rejects for any other reason */
size_t fa_cross_entropy_workspace_bytes(const fa_cross_entropy_params* s);
size_t fa_cross_entropy_params_size(void);

/*
 * fa_cross_entropy_bwd - the backward of fa_cross_entropy: one element-wise launch, no workspace.  From dlosses (fp32 [rows], any
 * element stride >= 0: a broadcast scalar is stride 0), the logits, the labels and the forward's lse, with the forward's scalars:
 *     g = dloss * logit_scale;   F = fma(2 * lse_square_scale, lse, 1);   p_j = exp(l_j - lse)
 *     dlogits_j = round_to_dtype(g * (((p_j * F) - (1 - label_smoothing) [j == label]) - label_smoothing / vocab))
 * Nothing but p_j is recomputed.  label == ignore_index: a row of +0; a label outside [0, vocab): a row of NaN.
 * dlogits: [rows, vocab] of `dtype` with its own row stride; it may be the logits tensor itself (the same base AND row stride: a
 * lane loads everything it owns before its first store); every other overlap of dlogits with an input is rejected.
 * No atomics, no host synchronisation, bitwise repeatable, capturable in a graph.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL dlosses, logits, labels, lse or dlogits; the dtype, vocab,
 * rows, row stride, alignment and scalar rules of fa_cross_entropy (for logits and dlogits alike); a negative dlosses_stride; a
 * dlogits that shares the logits' base but not their row stride; an illegal overlap; non-zero reserved fields.
 * rows x ceil(vocab / 8192) > 2^31 - 1: FA_ERR_UNSUPPORTED.  rows == 0: FA_OK without a launch.
 */
typedef struct fa_cross_entropy_bwd_params {
    size_t         struct_size;      /* sizeof(fa_cross_entropy_bwd_params) as the caller compiled it */
    const float*   dlosses;          /* device fp32: the gradient of losses; row r at dlosses[r * dlosses_stride] */
    const void*    logits;           /* [rows, vocab] of `dtype` */
    const int64_t* labels;           /* device [rows] */
    const float*   lse;              /* device [rows]: the forward's */
    void*          dlogits;          /* [rows, vocab] of `dtype`; may equal logits */
    int64_t        dlosses_stride;   /* elements, >= 0 */
    int64_t        logits_row_stride, dlogits_row_stride;   /* elements */
    int64_t        rows;
    int64_t        ignore_index;
    int32_t        vocab;
    int32_t        dtype;            /* FA_FP16, FA_BF16 or FA_FP32 */
    float          label_smoothing, logit_scale, lse_square_scale;   /* the forward's */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_cross_entropy_bwd_params;

int    fa_cross_entropy_bwd(const fa_cross_entropy_bwd_params* s, void* stream);
size_t fa_cross_entropy_bwd_params_size(void);

/*
 * fa_sample - token sampling from logits: temperature, top-k, min-p, top-p (in that order: the nucleus is taken over what the
 * other two leave, renormalised - the vLLM / HF order) and ONE inverse-CDF draw per row from a caller-supplied uniform number
 * (additive: fa_params and FA_ABI_VERSION are unchanged).  The serving-side end of the row ops: [rows, vocab] logits in, token
 * ids out.  logits: `dtype` FA_FP16, FA_BF16 or FA_FP32, last dimension contiguous, any row stride >= vocab (elements), element
 * alignment only.  The op holds no RNG: u is fp32 [rows], drawn by the caller (uniform in [0, 1)), so a call is deterministic and
 * capturable in a graph.  Each of the four parameters is a device [rows] array (fp32; top_k: int32) or, where the array is NULL,
 * the host value `*_value` for every row; both forms follow the same per-row rules, non-finite values included.
 *
 * Row r has raw values v_j = float(logits[r, j]), j < vocab; a NaN counts as -inf (and -0 as +0).  The ORDER: a before b iff
 * v_a > v_b, or v_a == v_b and a < b; j* is the first token in it.  Selection is on the raw values, exact whatever the temperature.
 *  1. Empty row: every v_j == -inf: id = -1, n_kept = 0, lse = -inf, a filtered row of -inf.  No address is formed from an id.
 *  2. Greedy: T = the row's temperature; the row is greedy when !(T > 0) (0, negative, NaN), when v_{j*} == +inf, or when T is
 *     so small that x_{j*} = v_{j*} * (1 / T) is not finite in fp32.  Then id = j*, n_kept = 1, the filtered row keeps j* alone
 *     and u is not read; lse is taken at inv_t = 1 for !(T > 0) (a row that holds +inf: NaN) and is not finite in the overflow
 *     case.  T = +inf is sampled with inv_t = 0: uniform over the tokens above -inf (a -inf logit has x = NaN: mass 0, lse NaN).
 *  3. Masses: otherwise inv_t = 1 / T (fp32); x_j = v_j * inv_t (ONE rounding); m = x_{j*}; e_j = e(x_j - m), e(t) = exp2(t *
 *     log2(e)): one fp32 product, one hardware exp2 (csrc/fa_lse.h).  The INTEGER MASS q_j = floor(e_j * 2^40) as an unsigned
 *     64-bit value (0 for -inf; q_{j*} = 2^40).  Everything below is integer arithmetic on the q_j: sums of up to 2^20 of them fit
 *     64 bits and do not depend on the order of addition, so a result cannot depend on the launch plan, rows or the row's index.
 *  4. Filters, each the length of a kept PREFIX of the order; n0 = the number of tokens above -inf.
 *       top_k:  n1 = k if 1 <= k < n0, else n0.
 *       min_p:  on when min_p > 0 (a NaN is off); mp = min(min_p, 1); n2 = the number of tokens among the first n1 with
 *               e_j >= mp (fp32 compare) - a prefix that holds at least j*.  Off: n2 = n1.
 *       top_p:  on when top_p < 1 (a NaN is off); Q2 = the sum of q over the first n2, Tq = max(1, ceil((double)top_p *
 *               (double)Q2)); n3 = the smallest n whose first-n mass is >= Tq (top_p <= 0 keeps one token).  Off: n3 = n2.
 *     Tokens tied at a cut enter in index order.
 *  5. Draw: Q = the sum of q over the kept set (the first n3); uu = u with a NaN or a negative value read as 0;
 *     rr = min(floor((double)uu * (double)Q), Q - 1); id = the kept token of smallest INDEX whose index-order running sum of kept
 *     q exceeds rr.
 *  6. Outputs, each optional (NULL: not written) but at least one of ids / filtered must be given:
 *       ids      int32 [rows]
 *       n_kept   int32 [rows]: n3 (greedy: 1, empty: 0)
 *       lse      fp32 [rows]: m + log(s) of fa_lse.h's running (max, sum-exp) over x in a fixed order - bitwise repeatable; the
 *                caller's log-probability of the UNFILTERED distribution is x_id - lse
 *       filtered [rows, vocab] of `dtype`, its own row stride: the logit's own bits where kept, -inf elsewhere.  Not in place.
 *     u may be NULL only where ids is NULL, or where temperature is NULL and !(temperature_value > 0).
 * Launch plan, a function of vocab alone.  vocab < 32768: one workgroup of 1024 lanes per row, one launch, no workspace.  vocab >=
 * 32768 (the split plan): a row is cut into ceil(vocab / 16384) chunks, one workgroup each, and every step that meets over the whole
 * row is a launch of its own on the stream - chunk statistics; then, as often as the longest row can need (a function of the dtype
 * and of which filters can be on), a sweep over the chunks followed by a one-workgroup-per-row step that takes its result and
 * decides the row's next sweep; then `filtered`.  The chunks' integer histograms and sums meet in the workspace by integer atomic
 * adds, the float partials of lse are merged in chunk order; no workgroup waits for another and the workspace needs no
 * initialisation.  fa_sample_workspace_bytes() = rows x (3392 + 160 x chunks, rounded up to 256) bytes there.  In both plans a row
 * is swept once for the statistics, once for the masses (min_p, or top_p without top_k), once per 8 key bits for each of top_k and
 * top_p (16-bit logits: 2 sweeps, fp32: 4: a radix select over the order-preserving integer key of v_j with a 256-bin histogram
 * of counts and masses), once for a tied class that is cut, once for the draw and once for `filtered`; a sweep that a row does
 * not need is left out (split plan: its workgroups leave at once).  Every loop's trip count is a function of vocab alone.  No
 * float atomics, no host synchronisation; a row's bits depend on (vocab, dtype), its values and its parameters alone.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL logits; neither ids nor filtered; a missing u; a dtype
 * other than FA_FP16 / FA_BF16 / FA_FP32; vocab < 1; negative rows or row strides, or (rows > 1) a row stride below vocab; logits
 * / filtered not aligned to their element, a [rows] array not 4-byte aligned, a workspace not 16-byte aligned or smaller than
 * reported; an output that overlaps an input, another output or the workspace; non-zero reserved fields.  vocab > 2^20 or
 * rows > 2^31 - 1: FA_ERR_UNSUPPORTED.  rows == 0: FA_OK without a launch.
 * Not covered: repetition / presence / frequency penalties and logit bias; an in-kernel RNG and per-row seeds; top-n log-prob
 * outputs; typical-p and the like; vocab > 2^20; in-place `filtered`.  (Rejection sampling and draft-tree verification for
 * speculative decoding: fa_spec_accept / fa_spec_walk below.)
 */
typedef struct fa_sample_params {
    size_t         struct_size;      /* sizeof(fa_sample_params) as the caller compiled it */
    const void*    logits;           /* [rows, vocab] of `dtype` */
    const float*   u;                /* device fp32 [rows]: one uniform number in [0, 1) per row */
    const float*   temperature;      /* device fp32 [rows], or NULL: temperature_value */
    const int32_t* top_k;            /* device int32 [rows], or NULL: top_k_value */
    const float*   top_p;            /* device fp32 [rows], or NULL: top_p_value */
    const float*   min_p;            /* device fp32 [rows], or NULL: min_p_value */
    int32_t*       ids;              /* device [rows], or NULL */
    int32_t*       n_kept;           /* device [rows], or NULL */
    float*         lse;              /* device [rows], or NULL */
    void*          filtered;         /* [rows, vocab] of `dtype`, or NULL */
    void*          workspace;        /* fa_sample_workspace_bytes() bytes, 16-byte aligned; may be NULL where that is 0 */
    size_t         workspace_bytes;
    int64_t        logits_row_stride, filtered_row_stride;   /* elements */
    int64_t        rows;
    int32_t        vocab;            /* 1 .. 2^20 */
    int32_t        dtype;            /* FA_FP16, FA_BF16 or FA_FP32 */
    float          temperature_value;    /* !(T > 0): greedy */
    int32_t        top_k_value;      /* < 1 or >= n0: off */
    float          top_p_value;      /* >= 1 or NaN: off */
    float          min_p_value;      /* <= 0 or NaN: off */
    int64_t        reserved[4];      /* 0 */
} fa_sample_params;

int    fa_sample(const fa_sample_params* s, void* stream);
/* the workspace of that call: a function of (rows, vocab, dtype) and of which filters can be on; `workspace`, `workspace_bytes` and
 * where the tensors lie are not looked at; 0 for a block that the call rejects for any other reason */
size_t fa_sample_workspace_bytes(const fa_sample_params* s);
size_t fa_sample_params_size(void);

/*
 * fa_spec_accept / fa_spec_walk - speculative-decoding verification: the rejection-sampling decision per draft node and the walk
 * that turns the decisions into the emitted tokens and the accepted path (additive: fa_params and FA_ABI_VERSION are unchanged).
 * What stands between fa_fwd_kvcache_tree (the draft chain or tree scored in one pass), fa_sample (ids from logits) and the commit
 * of the accepted path (fa_kv_gather + fa_kv_store by slot).  Neither op holds an RNG: the uniform numbers are the caller's.
 *
 * The data model.  A request has `nodes` = T nodes, 1 <= T <= 64: the query tokens of the tree-attention call.  Node 0 is the root,
 * the last token that is already accepted.  Node t >= 1 has parents[t] in [0, t); any other value (negative, or >= t) marks a
 * PADDING node, which is never visited - ragged draft lengths inside a fixed-shape batch.  parents is int32, request b's at
 * parents + b x parents_batch_stride (0: one tree for every request); NULL: the chain parents[t] = t - 1.  parents[0] is not
 * read.  draft_ids is int32 [batch, T] (entry 0 is not read).  Row (b, t) of a [batch x T, vocab] tensor is row b T + t.
 *
 * fa_spec_accept: per node t >= 1 that is no padding node, from the TARGET row P = (b, parents[t]) of target_logits (`dtype`
 * FA_FP16 / FA_BF16 / FA_FP32; it may hold fa_sample's `filtered` output: -inf outside a kept set) and the DRAFT row (b, t) of
 * draft_probs (`probs_dtype`, one of the same three; q_j = float(draft_probs[(b, t), j]) as it is, never renormalised), with
 * d = draft_ids[b, t] and T_b = request b's temperature (temperature[b], or temperature_value where the array is NULL):
 *  1. The target row's values v_j, the order, j*, "empty" and "greedy" are fa_sample's (rules 1 and 2 above, with T_b).
 *       empty row:   accept = 0, recovered = -1.
 *       greedy row:  (!(T_b > 0), v_{j*} = +inf, or x_{j*} not finite):  accept = (d == j*), recovered = j*; q and the uniform
 *                    numbers are not read.
 *  2. Masses, otherwise: inv_t, x_j, m = x_{j*} and e_j exactly as in fa_sample's rule 3.  s = the sum-exp of fa_lse.h's running
 *     (max, sum-exp) pair over x in this op's fixed order (8-column pieces in column order; a lane's pieces; the wave butterfly;
 *     the waves of a chunk in index order; the chunks in index order) - its maximum IS m.  p_j = e_j * (1.0f / s): one fp32 division
 *     for the row, one product per token.
 *  3. Accept: uu = u_accept[b T + t] with a NaN or a negative value read as 0; accept = (uu * q_d < p_d): one fp32 product, one
 *     compare (a NaN q_d rejects).  d outside [0, vocab): accept = 0, and no address is formed from d.
 *  4. Recovered token: r_j = min(max(p_j - q_j, 0), 1) - one fp32 subtraction; a NaN difference counts as 0 (the cap at 1 can
 *     only bind where q_j < 0).  The integer mass R_j = floor(r_j * 2^40) (uint64), R = the sum of the R_j: integer, so
 *     order-free.  If R == 0 (q covers p everywhere): R_j := floor(e_j * 2^40), fa_sample's q_j - the target's own masses.
 *     uu_r = u_recover[b T + t] read like uu; rr = min(floor((double)uu_r * (double)R), R - 1); recovered = the smallest index
 *     whose index-order running sum of R_j exceeds rr.
 *  Node 0 and padding nodes: accept = 0, recovered = -1.  Every element of accept / recovered (int32 [batch x T]) is written.
 * Launch plan, a function of vocab alone: a row is cut into C = ceil(vocab / 16384) chunks, one workgroup of 1024 lanes each, and
 * three kernels follow each other on the stream - (1) batch x T x C workgroups: the chunk's (m, s), first maximum and count of
 * values above -inf over the target row, one 32-byte partial each (plain stores); (2) batch x T x C workgroups: every chunk merges
 * the node's partials in chunk order (so all get the same m and s) and writes the chunk's sum of R_j and of floor(e_j 2^40)
 * (plain stores); (3) batch x T workgroups: the node's totals, the accept test (two element loads), the chunk that holds rr, and
 * one sweep of that chunk for the index.  A piece is one 16-byte load (fp32: two) where the row starts on a 16-byte boundary and
 * the piece lies inside the row, element loads otherwise: the same bits.  No float atomics, no workgroup waits for another, the
 * workspace needs no initialisation: fa_spec_accept_workspace_bytes() = batch x T x (48 x C rounded up to 64) bytes.  A node's
 * result depends on (vocab, the dtypes), its two rows, d, T_b and its two uniform numbers alone.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL target_logits, draft_probs, draft_ids, accept or
 * recovered; a missing u_accept / u_recover (they may be NULL only where temperature is NULL and !(temperature_value > 0)); a
 * dtype other than the three; nodes outside 1 .. 64; vocab < 1; a negative batch or stride, or (batch x T > 1) a row stride below
 * vocab; rows not aligned to their element, an int32 / fp32 array not 4-byte aligned, a workspace not 16-byte aligned or smaller
 * than reported; an output that overlaps an input, the other output or the workspace; non-zero reserved fields.  vocab > 2^20 or
 * more than 2^31 - 1 workgroups: FA_ERR_UNSUPPORTED.  batch == 0: FA_OK without a launch.
 *
 * fa_spec_walk: one wave per request, lane t owns node t, at most T steps whatever the data (a step ends the walk or moves to a
 * node of higher index).  c = 0; target_ids is int32, node t of request b at target_ids[b x target_ids_batch_stride + t x
 * target_ids_node_stride] (node stride 0: one id per request - a chain's bonus token).
 *   accept == NULL (deterministic drafts; recovered must be NULL too): emit y = target_ids[c]; if y == -1 stop; t = the child of c
 *     of LOWEST index with draft_ids[t] == y; none: stop; else append t to the path, c = t, repeat.
 *   accept given (with recovered: fa_spec_accept's outputs): t = the child of c of lowest index - its siblings are NOT looked at;
 *     none: emit target_ids[c] (the bonus token), stop; accept[t] != 0: emit draft_ids[t], append t, c = t, repeat; else emit
 *     recovered[t], stop.
 * Outputs, int32, every element written: out_tokens [batch, T] - the emitted tokens in order, then -1; num_out [batch] - their
 * number, 1 .. T; path_nodes [batch, T] - 0, t_1, t_2, .. (the accepted nodes, root included), then -1.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL draft_ids, target_ids or output; accept without recovered
 * or the reverse; nodes outside 1 .. 64; a negative batch or stride; an array not 4-byte aligned; an output that overlaps an input
 * or another output; non-zero reserved fields.  batch == 0: FA_OK without a launch.
 * Not covered: multi-child trees with draft probabilities (SpecInfer's multi-round rule: with draft_probs only the first child
 * of a node is tried); typical acceptance; an in-kernel RNG; a fused commit of the accepted path into the cache; vocab > 2^20.
 */
typedef struct fa_spec_accept_params {
    size_t         struct_size;      /* sizeof(fa_spec_accept_params) as the caller compiled it */
    const void*    target_logits;    /* [batch x nodes, vocab] of `dtype` */
    const void*    draft_probs;      /* [batch x nodes, vocab] of `probs_dtype` */
    const int32_t* draft_ids;        /* device int32 [batch, nodes] */
    const int32_t* parents;          /* device int32, or NULL: the chain */
    const float*   u_accept;         /* device fp32 [batch x nodes] */
    const float*   u_recover;        /* device fp32 [batch x nodes] */
    const float*   temperature;      /* device fp32 [batch], or NULL: temperature_value */
    int32_t*       accept;           /* device [batch x nodes], written */
    int32_t*       recovered;        /* device [batch x nodes], written */
    void*          workspace;        /* fa_spec_accept_workspace_bytes() bytes, 16-byte aligned */
    size_t         workspace_bytes;
    int64_t        logits_row_stride, probs_row_stride;   /* elements */
    int64_t        parents_batch_stride;                  /* elements; 0: one tree for every request */
    int64_t        batch;
    int32_t        nodes;            /* 1 .. 64 */
    int32_t        vocab;            /* 1 .. 2^20 */
    int32_t        dtype;            /* FA_FP16, FA_BF16 or FA_FP32 */
    int32_t        probs_dtype;      /* FA_FP16, FA_BF16 or FA_FP32 */
    float          temperature_value;    /* !(T > 0): greedy */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_spec_accept_params;

int    fa_spec_accept(const fa_spec_accept_params* s, void* stream);
/* the workspace of that call: a function of (batch, nodes, vocab) alone; `workspace`, `workspace_bytes` and where the tensors lie
 * are not looked at; 0 for a block that the call rejects for any other reason */
size_t fa_spec_accept_workspace_bytes(const fa_spec_accept_params* s);
size_t fa_spec_accept_params_size(void);

typedef struct fa_spec_walk_params {
    size_t         struct_size;      /* sizeof(fa_spec_walk_params) as the caller compiled it */
    const int32_t* parents;          /* device int32, or NULL: the chain */
    const int32_t* draft_ids;        /* device int32 [batch, nodes] */
    const int32_t* target_ids;       /* device int32, strided (below) */
    const int32_t* accept;           /* device int32 [batch x nodes], or NULL: deterministic drafts */
    const int32_t* recovered;        /* device int32 [batch x nodes]; NULL exactly where accept is */
    int32_t*       out_tokens;       /* device [batch, nodes], written */
    int32_t*       num_out;          /* device [batch], written */
    int32_t*       path_nodes;       /* device [batch, nodes], written */
    int64_t        parents_batch_stride;                           /* elements; 0: one tree for every request */
    int64_t        target_ids_batch_stride, target_ids_node_stride;   /* elements */
    int64_t        batch;
    int32_t        nodes;            /* 1 .. 64 */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_spec_walk_params;

int    fa_spec_walk(const fa_spec_walk_params* s, void* stream);
size_t fa_spec_walk_params_size(void);

/*
 * fa_act_mul - the gated activation of the MLP, act(gate) * up: SwiGLU, GeGLU and their ungated forms, forward (additive:
 * fa_params and FA_ABI_VERSION are unchanged).  gate, up, out: [rows, n] of `dtype` (FA_FP16 or FA_BF16), last dimension
 * contiguous, each with a row stride of its own >= n (elements).  The packed [rows, 2 n] form needs nothing more: gate = base,
 * up = base + n, both row strides 2 n.  All arithmetic is fp32 with ONE rounding to `dtype`:
 *     g = float(gate_j), u = float(up_j);   out_j = round(act(g) * u);   up == NULL (ungated): out_j = round(act(g))
 * act and its derivative, in exactly this fp32 order (every operation rounds once; fma is one rounding):
 *     e(t) = exp2(t * log2e) on the hardware exp2, log2e rounded to fp32;   sig(t) = rcp(1 + e(-t)) on the hardware reciprocal
 *     FA_ACT_SILU       s = sig(g);   act = g * s;   act' = s * fma(g, 1 - s, 1)
 *     FA_ACT_GELU_TANH  q = g * g;   w = (K2 * g) * fma(C3, q, 1);   s = sig(w);   act = g * s
 *                       act' = s * fma(g * (1 - s), K2 * fma(3 C3, q, 1), 1)
 *                       K2 = 2 sqrt(2 / pi), C3 = 0.044715, 3 C3 = 0.134145 as fp32 (0.5 (1 + tanh z) = sig(2 z): no tanh, no 1 + t)
 *     FA_ACT_GELU       ph = fma(0.5, erff(g * sqrt(1/2)), 0.5);   act = g * ph
 *                       act' = fma(g, e((g * g) * -0.5) * sqrt(1 / (2 pi)), ph)
 *     FA_ACT_RELU       act = g <= 0 ? +0 : g (a NaN stays a NaN);   act' = g <= 0 ? 0 : (g > 0 ? 1 : g)
 *     FA_ACT_RELU2      r = relu(g);   act = r * r;   act' = r + r
 * Special values are what these lines give literally: act(-100) = -0 for SILU and both GELUs (e overflows to +inf, rcp(+inf) = 0),
 * never NaN; a gate of -inf gives NaN there (-inf * 0) and +0 for the ReLUs; a NaN gate gives NaN.
 * A row is cut into runs of equal length (at most 8192 columns, whole waves of 8-column pieces); one workgroup of 256 lanes takes a
 * run, and a lane loads a piece from every input before it stores to it; no other lane touches it.  So out may be EXACTLY gate or EXACTLY up
 * (the same base address and row stride); every other overlap of out with an input is rejected.  The two halves of one packed
 * tensor - the same row stride, disjoint column ranges - do not overlap.  A row that does not start on a 16-byte boundary, and
 * the last n % 8 columns, are taken element by element: the same bits.  An element's bits depend on its own operands alone.
 * One launch, no workspace, no LDS, no atomics, no host synchronisation, capturable in a graph.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL gate or out; a dtype other than FA_FP16 / FA_BF16; an
 * unknown activation; n < 1; negative rows or row strides, or (rows > 1) a row stride below n; a pointer that is not 2-byte
 * aligned; an illegal overlap; non-zero reserved fields.  rows x runs per row > 2^31 - 1: FA_ERR_UNSUPPORTED.  rows == 0: FA_OK
 * without a launch.
 */
typedef enum fa_act {
    FA_ACT_SILU = 0,
    FA_ACT_GELU = 1,        /* the erf form */
    FA_ACT_GELU_TANH = 2,
    FA_ACT_RELU = 3,
    FA_ACT_RELU2 = 4        /* squared ReLU */
} fa_act;

typedef struct fa_act_mul_params {
    size_t         struct_size;      /* sizeof(fa_act_mul_params) as the caller compiled it */
    const void*    gate;             /* [rows, n] of `dtype` */
    const void*    up;               /* [rows, n] of `dtype`; NULL: the ungated form */
    void*          out;              /* [rows, n] of `dtype`; may equal gate or up */
    int64_t        gate_row_stride, up_row_stride, out_row_stride;   /* elements; up_row_stride is not read where up is NULL */
    int64_t        rows;
    int32_t        n;                /* >= 1 */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        activation;       /* fa_act */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_act_mul_params;

int    fa_act_mul(const fa_act_mul_params* s, void* stream);
size_t fa_act_mul_params_size(void);
/* the launch plan, a function of (rows, n) alone; needs no device.  run_columns: the columns of one run of a row (a multiple of
 * 512), items = rows x ceil(n / run_columns), grid = min(items, the cap): a workgroup strides over items.  Each output pointer may
 * be NULL.  FA_ERR_INVALID_ARGUMENT: rows < 0 or n < 1; FA_ERR_UNSUPPORTED: items > 2^31 - 1. */
int    fa_act_mul_plan(int64_t rows, int32_t n, int64_t* run_columns, int64_t* items, int64_t* grid);

/*
 * fa_act_mul_bwd - the backward of fa_act_mul: one element-wise launch with fa_act_mul's plan, no workspace.  It reads dout, gate
 * and up - the forward saves nothing but its inputs - and writes, with d = float(dout_j) and act / act' as above:
 *     dgate_j = round((d * u) * act'(g))        up == NULL: round(d * act'(g))
 *     dup_j   = round(d * act(g))               up == NULL: dup must be NULL too, and nothing is written for it
 * Every tensor is [rows, n] of `dtype` with a row stride of its own.  dgate may be EXACTLY gate and dup EXACTLY up (the same base
 * address and row stride: the backward in place, which needs no memory); dgate and dup may be the two halves of one packed
 * [rows, 2 n] gradient.  Every other overlap of an output with an input or with the other output is rejected.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL dout, gate or dgate; dup NULL while up is not, or the
 * reverse; the dtype, activation, n, rows, row stride and alignment rules of fa_act_mul; an illegal overlap; non-zero reserved
 * fields.  rows x runs per row > 2^31 - 1: FA_ERR_UNSUPPORTED.  rows == 0: FA_OK without a launch.
 */
typedef struct fa_act_mul_bwd_params {
    size_t         struct_size;      /* sizeof(fa_act_mul_bwd_params) as the caller compiled it */
    const void*    dout;             /* [rows, n]: the gradient of out */
    const void*    gate;             /* the forward's */
    const void*    up;               /* the forward's; NULL: ungated */
    void*          dgate;            /* [rows, n]; may equal gate */
    void*          dup;              /* [rows, n]; may equal up; NULL exactly where up is */
    int64_t        dout_row_stride, gate_row_stride, up_row_stride, dgate_row_stride, dup_row_stride;   /* elements */
    int64_t        rows;
    int32_t        n;
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        activation;       /* fa_act */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_act_mul_bwd_params;

int    fa_act_mul_bwd(const fa_act_mul_bwd_params* s, void* stream);
size_t fa_act_mul_bwd_params_size(void);

/*
 * fa_quant_fp8, fa_add_norm_quant, fa_act_mul_quant - dynamic fp8-e4m3 (OCP, "e4m3fn") quantisation of 16-bit activations, alone
 * and fused behind fa_add_norm's forward and fa_act_mul's forward (additive: fa_params and FA_ABI_VERSION are unchanged).  One
 * rule in all three, fp32 throughout; y_j are the values to quantise AFTER their rounding to `dtype` (fa_quant_fp8: x itself):
 *     a      = fmaxf(+0, |y_0|, |y_1|, ..)   over the row (FA_QUANT_ROW) or over each aligned group of 128 columns (FA_QUANT_GROUP);
 *                                            exact and order-free; fmaxf skips a NaN, so a row of NaNs alone has a = +0
 *     a'     = has_scale_ub ? fminf(a, scale_ub) : a
 *     scale  = fmaxf(a' / 448.0f, 0x1p-64f)  one IEEE division; the floor keeps 1 / scale finite for an all-zero row
 *     inv    = 1.0f / scale                  one IEEE division
 *     code_j = e4m3(fminf(fmaxf(y_j * inv, -448), 448))      the hardware conversion: round to nearest even, saturating
 * FA_QUANT_STATIC: `scale` is given by the caller (finite, > 0), only the last two lines run and no scale is written - the rule
 * fa_kv_store and the kv-cache append write fp8 caches with (csrc/fa_fp8_cvt.h), and what the fp8 q / k / v forward reads.
 * codes: [rows, n] bytes with a row stride of their own (>= n).  scales: fp32, contiguous - [rows] (ROW) or [rows, n / 128] (GROUP).
 * Fused means bit-identical to unfused: fa_add_norm_quant leaves the codes and scales of fa_quant_fp8 on fa_add_norm's `out`
 * (and fa_add_norm's residual_out), fa_act_mul_quant those of fa_quant_fp8 on fa_act_mul's `out` - the same arithmetic in the
 * same order, rounded to `dtype`, then the rule above.  The 16-bit `out` itself is not written.
 * Special values are what the lines above give literally; none is a fault, a device assert or a host synchronisation:
 *     an all-zero row (group)      a = 0, scale = 2^-64 (the floor), every code +0 or -0 with y's sign
 *     y_j = NaN                    skipped by a; its own code: NaN * inv = NaN, fmaxf(NaN, -448) = -448 -> the code of -448 (0xFE);
 *                                  the other codes and the scale are those of the row without it
 *     y_j = +-inf, no scale_ub     a = +inf, scale = +inf (stored), inv = 0: every finite y gives +-0, the infinite ones
 *                                  inf * 0 = NaN -> 0xFE
 *     y_j = +-inf, scale_ub        a' = scale_ub, the scale is finite: +-inf saturates to +-448 (0x7E / 0xFE)
 *     FA_QUANT_STATIC              NaN -> 0xFE, +-inf -> +-448
 * fa_quant_fp8: x [rows, n] of `dtype`, last dimension contiguous, any row stride >= n; n a multiple of 8 in [8, 65536] (GROUP: of
 *   128).  x is read once: a row (n > 512: one workgroup per row; below, 256 / G rows per workgroup, G lanes a row) stays in
 *   registers between the amax and the conversion.  A row of x that does not start on a 16-byte boundary, and a row of codes that
 *   does not start on an 8-byte boundary, are taken element by element: the same bits.
 * fa_add_norm_quant: fa_add_norm's forward - every field of `norm` as there, both of its forms (n <= 256 and wide) with its
 *   ownership and the order of its sums - except that norm.out must be NULL (norm.out_row_stride 0): codes and scales take its
 *   place.  residual_out is written as before; residual_out == residual stays legal.  codes: 8-byte aligned base and row stride.
 * fa_act_mul_quant: act(gate) * up (up NULL: act(gate)) with fa_act_mul's activations and fp32 order; gate, up as there but n a
 *   multiple of 8 in [8, 65536].  One workgroup owns a whole row in every mode (256 lanes up to 16384 columns, 1024 above, at
 *   most 8 pieces of 8 columns per lane and input).
 * One launch each, no workspace, no atomics, no host synchronisation, bitwise repeatable, capturable in a graph; a row's codes and
 * scale depend on that row alone.
 * FA_ERR_INVALID_ARGUMENT before any launch: a short struct_size; a NULL input or codes; scales NULL in ROW / GROUP or given in
 * STATIC; an unknown mode; a dtype other than FA_FP16 / FA_BF16; n not a multiple of 8 (GROUP: of 128) or outside the op's range;
 * negative rows or row strides, or (rows > 1) a row stride below n; a misaligned pointer (inputs: their element; scales: 4 bytes;
 * fa_add_norm_quant: fa_add_norm's rules); `scale` not finite and > 0 in STATIC, or not 0 elsewhere; has_scale_ub other than 0 / 1,
 * with STATIC, or with a scale_ub that is not finite and > 0 (scale_ub must be 0 where has_scale_ub is 0); any overlap of an output
 * with an input or another output (but residual_out == residual); fa_add_norm's and fa_act_mul's own rules; non-zero reserved
 * fields.  rows > 2^31 - 1: FA_ERR_UNSUPPORTED.  rows == 0: FA_OK without a launch.
 * Not covered: a backward or a straight-through estimator; device-resident static scales; per-tensor dynamic scales (a grid-wide
 * reduction); E8M0 / MX power-of-two scales; e5m2 and the fnuz formats; column-major or transposed scales and codes; fp4; fusing
 * into a GEMM; also writing the 16-bit out.
 */
typedef enum fa_quant_mode {
    FA_QUANT_ROW = 0,       /* one dynamic scale per row */
    FA_QUANT_GROUP = 1,     /* one dynamic scale per aligned group of 128 columns */
    FA_QUANT_STATIC = 2     /* the caller's scale; none is written */
} fa_quant_mode;

/* (mode, has_scale_ub, scale, scale_ub mean the same in the three blocks) */
typedef struct fa_quant_fp8_params {
    size_t         struct_size;      /* sizeof(fa_quant_fp8_params) as the caller compiled it */
    const void*    x;                /* [rows, n] of `dtype` */
    void*          codes;            /* [rows, n] fp8-e4m3 bytes */
    void*          scales;           /* fp32 [rows] (ROW), [rows, n / 128] (GROUP), NULL (STATIC) */
    int64_t        x_row_stride, codes_row_stride;       /* elements */
    int64_t        rows;
    int32_t        n;                /* a multiple of 8, 8 .. 65536; GROUP: of 128 */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        mode;             /* fa_quant_mode */
    int32_t        has_scale_ub;     /* 0 / 1; 0 in STATIC */
    float          scale;            /* STATIC: finite, > 0; otherwise 0 */
    float          scale_ub;         /* has_scale_ub: finite, > 0; otherwise 0 */
    int64_t        reserved[4];      /* 0 */
} fa_quant_fp8_params;

int    fa_quant_fp8(const fa_quant_fp8_params* s, void* stream);
size_t fa_quant_fp8_params_size(void);

typedef struct fa_add_norm_quant_params {
    size_t         struct_size;      /* sizeof(fa_add_norm_quant_params) as the caller compiled it */
    fa_add_norm_params norm;         /* fa_add_norm's block (its struct_size set); out NULL, out_row_stride 0 */
    void*          codes;            /* [rows, n] fp8-e4m3 bytes; 8-byte aligned */
    void*          scales;           /* fp32 [rows] (ROW), [rows, n / 128] (GROUP), NULL (STATIC) */
    int64_t        codes_row_stride; /* elements; a multiple of 8 */
    int32_t        mode;             /* fa_quant_mode */
    int32_t        has_scale_ub;     /* 0 / 1; 0 in STATIC */
    float          scale;            /* STATIC: finite, > 0; otherwise 0 */
    float          scale_ub;         /* has_scale_ub: finite, > 0; otherwise 0 */
    int64_t        reserved[4];      /* 0 */
} fa_add_norm_quant_params;

int    fa_add_norm_quant(const fa_add_norm_quant_params* s, void* stream);
size_t fa_add_norm_quant_params_size(void);

typedef struct fa_act_mul_quant_params {
    size_t         struct_size;      /* sizeof(fa_act_mul_quant_params) as the caller compiled it */
    const void*    gate;             /* [rows, n] of `dtype` */
    const void*    up;               /* [rows, n] of `dtype`; NULL: the ungated form */
    void*          codes;            /* [rows, n] fp8-e4m3 bytes */
    void*          scales;           /* fp32 [rows] (ROW), [rows, n / 128] (GROUP), NULL (STATIC) */
    int64_t        gate_row_stride, up_row_stride, codes_row_stride;   /* elements; up_row_stride is not read where up is NULL */
    int64_t        rows;
    int32_t        n;                /* a multiple of 8, 8 .. 65536; GROUP: of 128 */
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        activation;       /* fa_act */
    int32_t        mode;             /* fa_quant_mode */
    int32_t        has_scale_ub;     /* 0 / 1; 0 in STATIC */
    float          scale;            /* STATIC: finite, > 0; otherwise 0 */
    float          scale_ub;         /* has_scale_ub: finite, > 0; otherwise 0 */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_act_mul_quant_params;

int    fa_act_mul_quant(const fa_act_mul_quant_params* s, void* stream);
size_t fa_act_mul_quant_params_size(void);

/*
 * fa_moe_* - what surrounds the expert GEMMs of a mixture-of-experts block: top-k routing with its gradient, a stable counting
 * sort of the (token, k) slots by expert, the permutation of the activations into per-expert segments and the weighted combine
 * with its backward (additive: fa_params and FA_ABI_VERSION are unchanged).  The GEMMs themselves are not here: they see
 * contiguous, `align`-padded per-expert segments of `xp` described by expert_offsets.  No entry point synchronises with the host,
 * every result is a pure function of its inputs (no ordering depends on an atomic), all are capturable in a graph.
 * Limits, checked before any device work: tokens T >= 0; 2 <= num_experts E <= 512; 1 <= top_k K <= min(E, 16); hidden size n a
 * multiple of 8 in [8, 16384], fp16 / bf16; T * K + E * (align - 1) <= 2^31 - 1.  Outside them: FA_ERR_UNSUPPORTED.
 * FA_ERR_INVALID_ARGUMENT: a short struct_size, a NULL required pointer, an unknown dtype / scoring, a negative size or stride,
 * a row stride below the row's length (rows > 1), a misaligned pointer or stride (below), non-zero reserved fields, a workspace
 * smaller than the query's answer.
 *
 * fa_moe_route: logits [T, E] of `dtype` (FA_FP16, FA_BF16 or FA_FP32), last dimension contiguous, any row stride >= E.  One
 *   launch, no workspace, no atomics, no LDS.  A row lies 8 columns per lane in G adjacent lanes of a wave (G the smallest power
 *   of two with 8 G >= E; 64 / G rows per wave).  In fp32, every operation rounding once:
 *     FA_MOE_SOFTMAX  z_j = float(logit_j), a NaN read as -inf;  selection score c_j = z_j
 *     FA_MOE_SIGMOID  s_j = rcp(1 + exp2(-float(logit_j) * log2e)) (fa_act_mul's sigmoid: hardware exp2 and reciprocal);
 *                     c_j = s_j + bias_j (bias fp32 [E] or NULL: c_j = s_j), a NaN read as -inf
 *     selection       K rounds; round k takes the largest c_j not yet taken, the LOWEST index among equals (-0 == +0).  Slot k
 *                     holds the k-th winner: the ids of a row are distinct and inside [0, E) whatever the logits hold.
 *     softmax, renormalize      m = c_{id_0};  e_k = exp2((c_{id_k} - m) * log2e);  S = e_0 + e_1 + .. (ascending k);  w_k = e_k / S
 *     softmax, !renormalize     m = c_{id_0};  e_j = exp2((z_j - m) * log2e) for every column;  Z = the lane's columns added in
 *                               column order (absent columns +0), then the xor butterfly over the G lanes (m = 1, 2, ..);  w_k = e_{id_k} / Z
 *     sigmoid                   w_k = s_{id_k} (without the bias);  renormalize: S = w_0 + w_1 + .. (ascending k), w_k = w_k / S
 *     last                      w_k = w_k * scale.  The divisions are IEEE divisions.
 *   The order depends on (E, K, dtype) alone: a row's bits do not depend on T or on the row's index.  Special values follow
 *   these lines literally: an all -inf (or all-NaN softmax) row has ids 0 .. K - 1 and NaN weights (-inf - -inf); a +inf logit
 *   under softmax gives NaN weights for the row; a NaN logit under sigmoid loses the selection and, if it is selected all the
 *   same, has a NaN weight (and a NaN S).  weights: fp32 [T, K], ids: int32 [T, K], both contiguous.
 * fa_moe_route_bwd: dlogits [T, E] of `dtype` from dweights fp32 [T, K], the logits and the ids; nothing else is saved.  The
 *   selected scores are recomputed in the forward's order (m, e_k, S / Z, w_k as above), g_k = dweights_k * scale, and
 *     softmax, !renormalize     D = fma(g_k, p_k, D) ascending k from +0 (p = e / Z);  dl_j = p_j * (([j selected] ? g_j : 0) - D)
 *     softmax, renormalize      D as above with w;  dl_{id_k} = w_k * (g_k - D);  every other column +0
 *     sigmoid                   ds_k = g_k, or renormalize: D = fma(dweights_k, w_k, D), ds_k = ((dweights_k - D) * scale) / S;
 *                               dl_{id_k} = (ds_k * s_k) * (1 - s_k);  every other column +0
 *   with ONE rounding to `dtype`.  Every element of dlogits is written.  An id outside [0, E) is never used as an address: its
 *   slot counts as a logit of -inf.  bias does not enter the gradient and is not read.
 * fa_moe_sort: ids int32 [T * K] (slot s = t * K + k) -> sorted_slot int32 [M_max], pos int32 [T * K], expert_offsets int32
 *   [E + 1], M_max = T * K + E * (align - 1), 1 <= align <= 256.  Segment e starts at expert_offsets[e], a multiple of align, holds
 *   the slots with id e in ascending order and is padded with -1 to the next multiple of align; expert_offsets[E] is the padded
 *   total and everything from there to M_max is -1.  pos[s] is the slot's row, -1 for an id outside [0, E) (dropped: only ever
 *   compared).  Three launches over a workspace of fa_moe_sort_workspace_bytes (per-chunk expert counts): counts per chunk (LDS
 *   integer adds of pure counts), an exclusive scan, the placement by rank inside a wave (ballots) - no position comes from an
 *   atomic.  The plan is a function of (T * K, E) alone: fa_moe_sort_plan.
 * fa_moe_permute: out[r] = x[sorted_slot[r] / K] for r < rows (= M_max), a bit-exact copy; a row whose sorted_slot is outside
 *   [0, T * K) - the -1 padding - is +0.  With slot_scale (fp32 [T * K]): out[r] = round(slot_scale[s] * float(x[s / K])).
 *   sorted_slot NULL: every row is +0.  x, out: 16-byte aligned, row strides multiples of 8.
 * fa_moe_combine: out[t] = round(sum_k weights[t, k] * float(y[pos[t, k]])), acc = fma(w, y, acc) ascending k from +0, one
 *   rounding.  A pos outside [0, rows) - the -1 of a dropped slot - is skipped; a token without a live slot is +0.  weights NULL:
 *   every weight is 1 (the backward of fa_moe_permute).  A gather: no atomics.
 * fa_moe_combine_bwd: dy[pos[t, k]] = round(weights[t, k] * float(dout[t])) - fa_moe_permute's scaled product, bit for bit - over
 *   a dy set to +0 first (two launches; the pos of live slots are distinct, as fa_moe_sort leaves them), and
 *   dw[t, k] = sum_n float(dout[t, n]) * float(y[pos[t, k], n]) in the fixed order of the row sums of fa_add_norm (n <= 256: 8
 *   columns a lane, fma in column order, xor butterfly; above: 64 ceil(n / 512) <= 256 lanes, a lane's pieces added in ascending
 *   order, butterfly over the wave, waves added in index order); a dropped slot gets +0.  dy or dw NULL: not computed.
 */
typedef enum fa_moe_scoring {
    FA_MOE_SOFTMAX = 0,
    FA_MOE_SIGMOID = 1
} fa_moe_scoring;

typedef struct fa_moe_route_params {
    size_t         struct_size;      /* sizeof(fa_moe_route_params) as the caller compiled it */
    const void*    logits;           /* [tokens, num_experts] of `dtype` */
    const void*    bias;             /* fp32 [num_experts]; NULL: none.  FA_MOE_SIGMOID only */
    void*          weights;          /* fp32 [tokens, top_k], written */
    void*          ids;              /* int32 [tokens, top_k], written */
    int64_t        logits_row_stride;/* elements */
    int64_t        tokens;
    int32_t        num_experts, top_k;
    int32_t        dtype;            /* FA_FP16, FA_BF16 or FA_FP32 */
    int32_t        scoring;          /* fa_moe_scoring */
    int32_t        renormalize;      /* 0 / 1 */
    float          scale;            /* finite */
    int64_t        reserved[4];      /* 0 */
} fa_moe_route_params;

int    fa_moe_route(const fa_moe_route_params* s, void* stream);
size_t fa_moe_route_params_size(void);

typedef struct fa_moe_route_bwd_params {
    size_t         struct_size;      /* sizeof(fa_moe_route_bwd_params) as the caller compiled it */
    const void*    dweights;         /* fp32 [tokens, top_k] */
    const void*    logits;           /* the forward's */
    const void*    ids;              /* the forward's */
    void*          dlogits;          /* [tokens, num_experts] of `dtype`, every element written */
    int64_t        logits_row_stride, dlogits_row_stride;   /* elements */
    int64_t        tokens;
    int32_t        num_experts, top_k;
    int32_t        dtype;
    int32_t        scoring;
    int32_t        renormalize;
    float          scale;
    int64_t        reserved[4];      /* 0 */
} fa_moe_route_bwd_params;

int    fa_moe_route_bwd(const fa_moe_route_bwd_params* s, void* stream);
size_t fa_moe_route_bwd_params_size(void);

typedef struct fa_moe_sort_params {
    size_t         struct_size;      /* sizeof(fa_moe_sort_params) as the caller compiled it */
    const void*    ids;              /* int32 [tokens * top_k] */
    void*          sorted_slot;      /* int32 [tokens * top_k + num_experts * (align - 1)] */
    void*          pos;              /* int32 [tokens * top_k] */
    void*          expert_offsets;   /* int32 [num_experts + 1] */
    void*          workspace;        /* fa_moe_sort_workspace_bytes, 4-byte aligned */
    size_t         workspace_bytes;
    int64_t        tokens;
    int32_t        num_experts, top_k;
    int32_t        align;            /* 1 .. 256 */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_moe_sort_params;

int    fa_moe_sort(const fa_moe_sort_params* s, void* stream);
size_t fa_moe_sort_params_size(void);
size_t fa_moe_sort_workspace_bytes(const fa_moe_sort_params* s);   /* a function of (tokens * top_k, num_experts); no device */
/* the launch plan, a function of (slots = T * K, num_experts) alone; needs no device.  chunk_slots: the slots one wave counts and
 * places (a multiple of 64), chunks = max(1, ceil(slots / chunk_slots)) <= 1024, workspace_bytes = 4 * chunks * num_experts.
 * Each output pointer may be NULL. */
int    fa_moe_sort_plan(int64_t slots, int32_t num_experts, int64_t* chunk_slots, int64_t* chunks, int64_t* workspace_bytes);

typedef struct fa_moe_permute_params {
    size_t         struct_size;      /* sizeof(fa_moe_permute_params) as the caller compiled it */
    const void*    x;                /* [tokens, n] of `dtype` */
    const void*    sorted_slot;      /* int32 [rows]; NULL: every row +0 */
    const void*    slot_scale;       /* fp32 [tokens * top_k]; NULL: a copy */
    void*          out;              /* [rows, n] of `dtype` */
    int64_t        x_row_stride, out_row_stride;   /* elements, multiples of 8 */
    int64_t        rows;             /* M_max */
    int64_t        tokens;
    int32_t        top_k;
    int32_t        n;
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_moe_permute_params;

int    fa_moe_permute(const fa_moe_permute_params* s, void* stream);
size_t fa_moe_permute_params_size(void);

typedef struct fa_moe_combine_params {
    size_t         struct_size;      /* sizeof(fa_moe_combine_params) as the caller compiled it */
    const void*    y;                /* [rows, n] of `dtype` */
    const void*    weights;          /* fp32 [tokens, top_k]; NULL: ones */
    const void*    pos;              /* int32 [tokens, top_k] */
    void*          out;              /* [tokens, n] of `dtype` */
    int64_t        y_row_stride, out_row_stride;   /* elements, multiples of 8 */
    int64_t        rows;
    int64_t        tokens;
    int32_t        top_k;
    int32_t        n;
    int32_t        dtype;
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_moe_combine_params;

int    fa_moe_combine(const fa_moe_combine_params* s, void* stream);
size_t fa_moe_combine_params_size(void);

typedef struct fa_moe_combine_bwd_params {
    size_t         struct_size;      /* sizeof(fa_moe_combine_bwd_params) as the caller compiled it */
    const void*    dout;             /* [tokens, n] of `dtype` */
    const void*    y;                /* [rows, n]; read for dw only (may be NULL where dw is) */
    const void*    weights;          /* fp32 [tokens, top_k]; read for dy only (may be NULL where dy is) */
    const void*    pos;              /* int32 [tokens, top_k] */
    void*          dy;               /* [rows, n] of `dtype`; NULL: skipped */
    void*          dw;               /* fp32 [tokens, top_k]; NULL: skipped */
    int64_t        dout_row_stride, y_row_stride, dy_row_stride;   /* elements, multiples of 8 */
    int64_t        rows;
    int64_t        tokens;
    int32_t        top_k;
    int32_t        n;
    int32_t        dtype;
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_moe_combine_bwd_params;

int    fa_moe_combine_bwd(const fa_moe_combine_bwd_params* s, void* stream);
size_t fa_moe_combine_bwd_params_size(void);

/*
 * fa_moe_gemm: the grouped expert GEMM of a mixture-of-experts block, forward, fp16 / bf16 with fp32 accumulation
 * (csrc/fa_moe_gemm.hip).  One launch, no workspace, no atomics, no host synchronisation: expert_offsets (int32 [E + 1], as
 * fa_moe_sort writes it) stays on the device.  rows = M_max, the rows of out.
 *   segment rows   expert_offsets[e] <= r < expert_offsets[e + 1]:
 *                  out[r, n] = round(sum_k float(a_r[k]) * float(W_e[k, n]) (+ float(bias[e, n]))), fp32 accumulation, ONE rounding
 *   other rows     expert_offsets[E] <= r < rows: +0.  With expert_offsets[0] == 0 (fa_moe_sort's) every element of out is written
 *                  exactly once; rows below a positive expert_offsets[0] belong to no segment and are left unwritten.
 *   a_r            sorted_slot NULL: x[r], x being [rows, k] (fa_moe_permute's output).  sorted_slot (int32 [rows]) given: x is the
 *                  un-permuted [tokens, k] and a_r = x[sorted_slot[r] / top_k]; a slot outside [0, tokens * top_k) - the -1 padding -
 *                  reads as a row of +0 and forms no address.  fa_moe_gemm with sorted_slot has the bits of fa_moe_permute followed
 *                  by fa_moe_gemm.
 *   layout         FA_MOE_W_NK: w is [E, n, k] (W_e[k, n] = w[e, n, k], nn.Linear);  FA_MOE_W_KN: w is [E, k, n].  The "kn" call
 *                  with n and k exchanged is the data gradient of an "nk" layer.
 *   order          every output element has one accumulator chain of v_mfma_f32_32x32x16 over k ascending in steps of 16 from +0,
 *                  in every tile shape; the bias is added to the finished sum in fp32.  A row's bits are a function of its source
 *                  row, W_e, bias[e] and k alone - not of rows, of the row's place in its segment or of the other experts.
 *   tensors        w: 16-byte aligned, w_expert_stride >= n * k and a multiple of 8 (elements; every offset is 64-bit).  x, out:
 *                  16-byte aligned, row strides multiples of 8, at most 2^22, out's at least n.  bias: [E, n] contiguous of `dtype`
 *                  or FA_FP32 (bias_dtype), or NULL.
 *   limits         2 <= num_experts <= 512; n, k multiples of 8, n <= 65536, k <= 32768; 0 <= rows < 2^31 (rows == 0 launches
 *                  nothing); with sorted_slot 1 <= top_k <= 16 and tokens * top_k < 2^31.  Outside: FA_ERR_UNSUPPORTED, before
 *                  any device work.
 *   offsets        expert_offsets values are only compared and clamped to [0, rows]: a decreasing or out-of-range table gives
 *                  wrong rows, never an address outside out, x or w.
 * fa_moe_gemm_plan: the launch plan, a function of its arguments alone; needs no device.  block_m is 128 (prefill) or 32 (decode:
 *   rows <= 32 * num_experts), block_n 128, block_k 64; grid_m = floor(rows / block_m) + num_experts + 1 bounds the tiles that
 *   num_experts segments and the +0 tail can need (a workgroup finds its (expert, tile) from expert_offsets; one without a tile
 *   leaves), grid_n = ceil(n / block_n).  Each output pointer may be NULL.
 */
typedef enum fa_moe_w_layout {
    FA_MOE_W_NK = 0,
    FA_MOE_W_KN = 1
} fa_moe_w_layout;

typedef struct fa_moe_gemm_params {
    size_t         struct_size;      /* sizeof(fa_moe_gemm_params) as the caller compiled it */
    const void*    x;                /* [rows, k], or with sorted_slot [tokens, k], of `dtype` */
    const void*    w;                /* [num_experts, n, k] (FA_MOE_W_NK) or [num_experts, k, n] (FA_MOE_W_KN) of `dtype` */
    const void*    bias;             /* [num_experts, n] of `bias_dtype`, contiguous; NULL: none */
    const void*    expert_offsets;   /* int32 [num_experts + 1], device */
    const void*    sorted_slot;      /* int32 [rows]; NULL: the plain form */
    void*          out;              /* [rows, n] of `dtype` */
    int64_t        x_row_stride, out_row_stride;   /* elements, multiples of 8 */
    int64_t        w_expert_stride;  /* elements, >= n * k, a multiple of 8 */
    int64_t        rows;             /* M_max */
    int64_t        tokens;           /* rows of x with sorted_slot; ignored without */
    int32_t        num_experts, top_k;              /* top_k: with sorted_slot only */
    int32_t        n, k;
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        bias_dtype;       /* `dtype` or FA_FP32; ignored without bias */
    int32_t        layout;           /* fa_moe_w_layout */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_moe_gemm_params;

int    fa_moe_gemm(const fa_moe_gemm_params* s, void* stream);
size_t fa_moe_gemm_params_size(void);
int    fa_moe_gemm_plan(int64_t rows, int32_t n, int32_t k, int32_t num_experts, int32_t layout, int32_t dtype,
                        int32_t* block_m, int32_t* block_n, int32_t* block_k, int64_t* grid_m, int64_t* grid_n);

/*
 * fa_moe_gemm_wgrad: the weight gradient of fa_moe_gemm, and the bias gradient (csrc/fa_moe_gemm_wgrad.hip).  No workspace, no
 * atomics, no host synchronisation; expert_offsets is read as fa_moe_gemm reads it (clamped to [0, rows], only compared).
 *   dw             FA_MOE_W_NK: [E, n, k];  FA_MOE_W_KN: [E, k, n].  With L_e the rows expert_offsets[e] <= r < expert_offsets[e + 1],
 *                  dW_e[n, k] = round(sum_{r in L_e} float(dy[r, n]) * float(a_r[k])) (+ the old dw with accumulate), fp32
 *                  accumulation, ONE rounding.  An empty expert's dW is +0 (with accumulate: left as it is).  Rows in no
 *                  segment - below a positive expert_offsets[0], from expert_offsets[E] on - contribute nothing.
 *   a_r            as in fa_moe_gemm: x[r], or with sorted_slot x[sorted_slot[r] / top_k], a slot outside [0, tokens * top_k)
 *                  being a row of +0 that forms no address.
 *   dbias          [E, n] of dbias_dtype (`dtype` or FA_FP32), or NULL: round(sum_{r in L_e} float(dy[r, n])), +0 for an empty
 *                  expert.  A second, small launch: 16 fp32 partial sums per column (rows first + j, first + j + 16, ...
 *                  ascending), added in ascending j - an order that depends on the segment's length alone.  dw NULL: dbias alone.
 *   order          every element of dW is one accumulator chain of v_mfma_f32_32x32x16 from +0 over the segment's rows, from its
 *                  first row ascending in steps of 16: no split over rows.  A tile's bits are a function of its segment's rows
 *                  of dy and a alone - not of the other segments, of E, of where the segment lies, or of the tail.  Rows at or
 *                  behind a segment's end are never loaded (they are zero-filled): a NaN in a neighbouring segment stays there.
 *   tensors        dy [rows, n], x [rows, k] or [tokens, k]: 16-byte aligned, row strides multiples of 8, at least the row
 *                  length, at most 2^22.  dw: 16-byte aligned, of dw_dtype (`dtype`, or FA_FP32), dw_expert_stride >= n * k and a
 *                  multiple of 8 (elements).  accumulate != 0 (dw = dw + sum, one fp32 add; every element has one writer) needs
 *                  an FA_FP32 dw.
 *   limits         those of fa_moe_gemm, FA_ERR_UNSUPPORTED outside them before any device work.  rows == 0 still writes every
 *                  dW and dbias +0 (unless accumulating).
 * fa_moe_gemm_wgrad_plan: tile extents along n, along k and the rows staged per step (128, 128, 64) and the grid
 *   (ceil(n / 128), ceil(k / 128), num_experts): a function of the shapes alone.  Each output pointer may be NULL.
 */
typedef struct fa_moe_gemm_wgrad_params {
    size_t         struct_size;      /* sizeof(fa_moe_gemm_wgrad_params) as the caller compiled it */
    const void*    dy;               /* [rows, n] of `dtype` */
    const void*    x;                /* [rows, k], or with sorted_slot [tokens, k], of `dtype` */
    const void*    expert_offsets;   /* int32 [num_experts + 1], device */
    const void*    sorted_slot;      /* int32 [rows]; NULL: the plain form */
    void*          dw;               /* [num_experts, n, k] / [num_experts, k, n] of `dw_dtype`; NULL: not computed */
    void*          dbias;            /* [num_experts, n] of `dbias_dtype`, contiguous; NULL: not computed */
    int64_t        dy_row_stride, x_row_stride;    /* elements, multiples of 8 */
    int64_t        dw_expert_stride; /* elements, >= n * k, a multiple of 8 */
    int64_t        rows;             /* M_max */
    int64_t        tokens;           /* rows of x with sorted_slot; ignored without */
    int32_t        num_experts, top_k;              /* top_k: with sorted_slot only */
    int32_t        n, k;
    int32_t        dtype;            /* FA_FP16 or FA_BF16 */
    int32_t        dw_dtype;         /* `dtype` or FA_FP32 */
    int32_t        dbias_dtype;      /* `dtype` or FA_FP32; ignored without dbias */
    int32_t        layout;           /* fa_moe_w_layout */
    int32_t        accumulate;       /* != 0: dw += (FA_FP32 dw only) */
    int32_t        reserved0;        /* 0 */
    int64_t        reserved[4];      /* 0 */
} fa_moe_gemm_wgrad_params;

int    fa_moe_gemm_wgrad(const fa_moe_gemm_wgrad_params* s, void* stream);
size_t fa_moe_gemm_wgrad_params_size(void);
int    fa_moe_gemm_wgrad_plan(int32_t n, int32_t k, int32_t num_experts, int32_t layout, int32_t dtype,
                              int32_t* block_n, int32_t* block_k, int32_t* block_rows,
                              int64_t* grid_n, int64_t* grid_k, int64_t* grid_e);

/*
 * Row gather / scatter for the padding helpers on both sides of the varlen path (HBM-bound byte movement).
 * Rows are `row_bytes` bytes (a multiple of 16, 16-byte aligned base pointers), indices are int64 on the device
 * (negative values count from the end, as in torch); no bounds checks beyond that (same contract as the reference's
 * torch.gather / index assignment, flash_attn/bert_padding.py:9-60).
 *
 * fa_gather_rows : dst[i, :] = src[indices[i], :] for i < n_idx.  `src_row_stride_bytes` >= row_bytes lets the
 *   source be a row-strided view.  Replaces `index_first_axis` forward / `index_put_first_axis` backward
 *   (bert_padding.py:9-34, :52-60) as used by `unpad_input` (:79-104).
 * fa_scatter_rows: dst[:] = 0; dst[indices[i], :] = src[i, :].  With `sorted_unique` != 0 (indices ascending
 *   without repeats - what unpad_input produces) it is one pass over dst; otherwise memset + scatter (repeated
 *   indices: one of the rows wins, as in the reference).  Replaces `index_put_first_axis` forward /
 *   `index_first_axis` backward (bert_padding.py:36-50, :22-34) as used by `pad_input` (:135-146).
 */
int fa_gather_rows(const void* src, const int64_t* indices, void* dst, int64_t n_idx, int64_t row_bytes,
                   int64_t src_row_stride_bytes, int64_t n_src_rows, void* stream);
int fa_scatter_rows(const void* src, const int64_t* indices, void* dst, int64_t n_idx, int64_t n_dst_rows,
                    int64_t row_bytes, int sorted_unique, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA_MI355_H */
