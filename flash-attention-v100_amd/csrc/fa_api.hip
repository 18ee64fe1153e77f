// fa_api.hip - extern "C" entry points of libfa_mi355.so (see include/fa_mi355.h).
//
// Host-side validation and flag normalisation mirror the reference's wrappers:
//   dense    kernel/fused_mha_forward.cu:317-371,409-413
//   varlen   kernel/fused_mha_forward_varlen.cu:371-482
//   kvcache  kernel/fused_mha_forward_kvcache.cu:416-472,488,582-598
//   backward kernel/fused_mha_backward.cu:577-692, kernel/fused_mha_backward_varlen.cu:636-765
// Errors never cross the boundary as exceptions: negative status + fa_last_error().
#include <cstdarg>
#include <cstddef>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include "fa_common.h"
#include "fa_moe.h"                                   // fa_moe.hip: the limits, the sort plan and the launchers of fa_moe_*
#include "fa_moe_gemm.h"                              // fa_moe_gemm.hip: the limits, the launch plan and the launcher of fa_moe_gemm

namespace fa {
int launch_fwd(const KArgs& a, hipStream_t stream);
int launch_fwd_fp8(const KArgs& a, hipStream_t stream);  // fa_fwd_fp8.hip: fp8-e4m3 q, k, v
size_t fwd_split_workspace_bytes(const KArgs& a);        // fa_fwd_asm.hip: forward key split of one-wave causal launches
int launch_gather_rows(const void* src, const int64_t* idx, void* dst, int64_t n_idx, int64_t row_bytes,
                       int64_t src_stride, int64_t n_src_rows, hipStream_t stream);
int launch_scatter_rows(const void* src, const int64_t* idx, void* dst, int64_t n_idx, int64_t n_dst_rows,
                        int64_t row_bytes, int sorted_unique, hipStream_t stream);
int launch_bwd(const KArgs& a, hipStream_t stream);
int launch_bwd_dsinks(const KArgs& a, float* dsinks, hipStream_t stream);   // fa_bwd.hip: gradient of the attention sinks
size_t bwd_workspace_bytes(const fa_params& p, bool flat);
int launch_kvcache_append(const KArgs& a, hipStream_t stream);
int launch_decode(const KArgs& a, hipStream_t stream, const fa_tree_params* tree = nullptr);
size_t decode_workspace_bytes(const fa_params& p);
bool decode_applicable(const fa_params& p);
bool decode_takes(const fa_params& p);
int merge_vec_width(const fa_merge_params& m);           // fa_merge.hip: 8 / 4 values per piece, 0 = o not 8-byte aligned
void launch_merge_states(const fa_merge_params& m, hipStream_t stream);
void launch_rotary(const fa_rotary_params& r, hipStream_t stream);          // fa_rotary.hip: standalone rotary embedding
void launch_kv_store(const fa_kv_store_params& s, hipStream_t stream);      // fa_kv_store.hip: ragged K / V rows into a KV cache
void launch_kv_gather(const fa_kv_gather_params& s, hipStream_t stream);    // fa_kv_gather.hip: ragged K / V rows out of a KV cache
void launch_rope_store(const fa_rope_store_params& s, hipStream_t stream);  // fa_rope_store.hip: RoPE at per-token positions + K / V store
void launch_qk_norm_rope_store(const fa_qk_norm_rope_store_params& s, hipStream_t stream);   // fa_qk_norm_rope_store.hip: QK RMSNorm in front of that
void launch_qk_norm_rope_bwd(const fa_qk_norm_rope_bwd_params& s, hipStream_t stream);       // fa_qk_norm_rope_bwd.hip: its backward (dx, dw)
size_t qk_norm_rope_bwd_workspace_bytes(const fa_qk_norm_rope_bwd_params& s);                // the dw partial rows of its launch plan
void launch_add_norm(const fa_add_norm_params& s, hipStream_t stream);                       // fa_add_norm.hip: residual add + RMSNorm / LayerNorm
void launch_add_norm_bwd(const fa_add_norm_bwd_params& s, hipStream_t stream);               // fa_add_norm_bwd.hip: its backward (dx, dres, dweight, dbias)
size_t add_norm_bwd_workspace_bytes(const fa_add_norm_bwd_params& s);                        // the partial rows of its launch plan
void launch_cross_entropy(const fa_cross_entropy_params& s, hipStream_t stream);             // fa_cross_entropy.hip: softmax cross-entropy over the vocabulary
void launch_cross_entropy_bwd(const fa_cross_entropy_bwd_params& s, hipStream_t stream);     // its backward (dlogits)
size_t cross_entropy_workspace_bytes(int64_t rows, int vocab, int dtype);                    // the chunk partials of its launch plan
int64_t ce_nchunks(int vocab, int dtype);                                                    // forward / backward workgroups per row
int64_t ce_bwd_nchunks(int vocab);
void launch_sample(const fa_sample_params& s, hipStream_t stream);                           // fa_sample.hip: temperature / top-k / min-p / top-p token sampling
size_t sample_workspace_bytes(int64_t rows, int vocab, int dtype);                           // the per-row records, bins and partials of its split plan
int64_t sample_chunks_per_row(int vocab);                                                    // workgroups per row of its launch plan
void launch_spec_accept(const fa_spec_accept_params& s, hipStream_t stream);                 // fa_spec_verify.hip: rejection sampling per draft node
void launch_spec_walk(const fa_spec_walk_params& s, hipStream_t stream);                     // .. and the walk over the decisions
size_t spec_accept_workspace_bytes(int64_t rows, int vocab);                                 // the chunk partials and sums of its launch plan
int64_t spec_accept_chunks(int vocab);                                                       // workgroups per node of its launch plan
void launch_act_mul(const fa_act_mul_params& s, hipStream_t stream);                         // fa_act_mul.hip: act(gate) * up, element-wise
void launch_act_mul_bwd(const fa_act_mul_bwd_params& s, hipStream_t stream);                 // its backward (dgate, dup)
struct ActPlan { int chunk_pieces; int64_t nchunks, items; int grid; };                      // its launch plan: runs per row, items, grid
ActPlan act_plan(int64_t rows, int n);
void launch_quant_fp8(const fa_quant_fp8_params& s, hipStream_t stream);                     // fa_quant.hip: dynamic fp8-e4m3 quantisation of [rows, n]
void launch_add_norm_quant(const fa_add_norm_quant_params& s, hipStream_t stream);           // .. behind fa_add_norm's forward
void launch_act_mul_quant(const fa_act_mul_quant_params& s, hipStream_t stream);             // .. behind fa_act_mul's forward
}  // namespace fa

static thread_local std::string g_last_error;

static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define FA_CHECK(cond, ...)                                              \
    do {                                                                 \
        if (!(cond)) return fail(FA_ERR_INVALID_ARGUMENT, __VA_ARGS__);  \
    } while (0)

static int check_hip(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FA_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return FA_OK;
}

// Experiment switches, read ONCE (first call): FA_VARLEN_GRID=1 keeps the batch x max_seqlen grid for varlen.
static bool varlen_grid_env() {
    static const bool on = getenv("FA_VARLEN_GRID") != nullptr;
    return on;
}

static bool supported_head_dim(int d) { return d == 64 || d == 128 || d == 256; }

// Checks shared by every op (reference: fused_mha_forward.cu:324-340).  fp8_q: the op takes fp8-e4m3 q (fa_fwd, fa_varlen_fwd).
static int check_common(const fa_params& p, bool need_out, bool fp8_q = false) {
    const bool no_keys = (p.seqlen_k == 0 && !p.cu_seqlens_k);
    FA_CHECK(p.q && (no_keys || (p.k && p.v)), "q, k, v must not be NULL");
    FA_CHECK(!need_out || (p.o && p.lse), "o and lse must not be NULL");
    if (fp8_q)
        FA_CHECK(p.dtype == FA_FP16 || p.dtype == FA_BF16 || p.dtype == FA_FP8_E4M3, "q must be fp16 or bf16 (or fp8-e4m3 with fp8-e4m3 k/v)");
    else
        FA_CHECK(p.dtype == FA_FP16 || p.dtype == FA_BF16, "q must be fp16 or bf16");
    FA_CHECK((p.flags & ~(FA_FLAG_KEEP_WINDOW | FA_FLAG_NO_DKV_SPLIT | FA_FLAG_DS_HANDOFF | FA_FLAG_FWD_KEY_SPLIT)) == 0, "fa_params::flags has unknown bits set (zero-initialise the struct)");
    FA_CHECK(p.batch > 0, "batch size must be positive");
    FA_CHECK(p.head_dim <= 256, "head dimension must be <= 256");
    FA_CHECK(p.head_dim % 8 == 0, "head dimension must be multiple of 8");
    FA_CHECK(p.nheads_k > 0 && p.nheads_q % p.nheads_k == 0, "H_Q must be divisible by H_K for GQA/MQA");
    FA_CHECK(p.p_dropout >= 0.f && p.p_dropout < 1.f, "p_dropout must be in [0, 1)");
    if (p.softcap > 0.f) FA_CHECK(p.p_dropout == 0.f, "Softcapping does not support dropout for now");
    const int kv_al = p.kv_dtype == FA_FP8_E4M3 ? 16 : 8;
    const int q_al = p.dtype == FA_FP8_E4M3 ? 16 : 8;
    FA_CHECK((p.q_row_stride % q_al) == 0 && (p.q_head_stride % q_al) == 0 && (p.k_row_stride % kv_al) == 0 &&
             (p.k_head_stride % kv_al) == 0 && (p.v_row_stride % kv_al) == 0 && (p.v_head_stride % kv_al) == 0,
             "q/k/v strides must be multiples of 16 bytes");
    FA_CHECK((reinterpret_cast<uintptr_t>(p.q) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.k) & 15) == 0 &&
             (reinterpret_cast<uintptr_t>(p.v) & 15) == 0, "q/k/v must be 16-byte aligned");
    if (!supported_head_dim(p.head_dim))
        return fail(FA_ERR_UNSUPPORTED, "head dimension %d has no gfx950 kernel in this build (64, 128, 256)", p.head_dim);
    // The kernels address one (batch, head) slice through a buffer descriptor: 32-bit byte offsets.  Packed (varlen) tensors:
    // every kernel rebases its pointers at the sequence's first row in 64-bit arithmetic (q_row0 / k_row0 x row stride - the
    // reference offsets with size_t, include/template.h:199-217), so the slice is ONE SEQUENCE (max_seqlen rows), not the
    // total_q / total_k rows of the packed tensor; paged caches: one page.
    {
        const int64_t rows_q = p.seqlen_q;
        const int64_t rows_k = p.block_table ? p.page_block_size : p.seqlen_k;
        FA_CHECK(p.head_dim_v >= 0 && p.head_dim_v <= p.head_dim && p.head_dim_v % 8 == 0,
                 "head_dim_v must be a multiple of 8 in [0, head_dim]");
        const bool narrow = p.head_dim_v > 0 && p.head_dim_v < p.head_dim;
        const int64_t lim = (int64_t)1 << (narrow ? 31 : 32);
        // q: 2 GiB - its rows are fetched through one descriptor whose offset 0x80000000 must lie OUTSIDE the slice (rows past the
        // sequence and columns past the valid width come back as zeros from the range check)
        FA_CHECK(rows_q * p.q_row_stride * 2 < ((int64_t)1 << 31),
                 "one (batch / sequence, head) slice of q spans more than 2 GiB: not addressable by the gfx950 kernels");
        FA_CHECK(rows_k * p.k_row_stride * 2 < lim && rows_k * p.v_row_stride * 2 < lim,
                 "one (batch / sequence, head) slice of k/v spans more than 4 GiB: not addressable by the gfx950 kernels");
    }
    return FA_OK;
}

// Flag normalisation, the reference's (fused_mha_forward.cu:343-352): a window of >= seqlen_k keys is dropped.  For
// seqlen_q <= seqlen_k that cannot change a result.  For seqlen_q > seqlen_k a right window of seqlen_k <= wr < seqlen_q - 1
// keys still hides key j' > i + wr from the first rows and the reference un-masks them; the drop-in API does the same.
// FA_FLAG_KEEP_WINDOW (this library's context-parallel wrapper: all queries over a slice of the keys, the shard's causal
// offset as a right window) drops a right window only where it hides nothing.
static void normalize(fa_params& p, bool kvcache) {
    if (p.seqlen_q == 1 && !p.alibi_slopes) p.is_causal = 0;
    if (kvcache && p.is_causal) p.window_right = 0;
    if (p.window_left >= p.seqlen_k) p.window_left = -1;
    const bool keep = (p.flags & FA_FLAG_KEEP_WINDOW) != 0;
    if (p.window_right >= p.seqlen_k && (!keep || p.window_right >= p.seqlen_q - 1)) p.window_right = -1;
}

// fp8-e4m3 q, k, v (fa_fwd / fa_varlen_fwd, fa_fwd_fp8.hip): what the kernel covers, and descales of 0 turned into 1.0
static int check_fp8_q(fa_params& p) {
    FA_CHECK(p.kv_dtype == FA_FP8_E4M3, "fp8-e4m3 q needs fp8-e4m3 k and v");
    FA_CHECK(p.o_dtype == FA_FP16 || p.o_dtype == FA_BF16, "fp8-e4m3 q: o_dtype must be FA_FP16 or FA_BF16");
    float* ds[3] = {&p.q_descale, &p.k_descale, &p.v_descale};
    for (float* d : ds) {
        FA_CHECK(*d >= 0.f && *d <= 3.402823466e38f, "fp8-e4m3 q: q/k/v descales must be finite and >= 0 (0 = 1.0)");
        if (*d == 0.f) *d = 1.f;
    }
    if (p.alibi_slopes) return fail(FA_ERR_UNSUPPORTED, "fp8-e4m3 q: ALiBi is not supported");
    if (p.softcap > 0.f) return fail(FA_ERR_UNSUPPORTED, "fp8-e4m3 q: softcap is not supported");
    if (p.p_dropout > 0.f || p.dmask) return fail(FA_ERR_UNSUPPORTED, "fp8-e4m3 q: dropout is not supported");
    if (p.block_table) return fail(FA_ERR_UNSUPPORTED, "fp8-e4m3 q: paged K/V is not supported");
    if (p.head_dim > 128) return fail(FA_ERR_UNSUPPORTED, "fp8-e4m3 q: head dimension %d is not supported (64, 128)", p.head_dim);
    FA_CHECK(p.head_dim_v % 16 == 0, "fp8-e4m3 q: head_dim_v must be a multiple of 16");
    return FA_OK;
}

// fa_ext_params (the *_ext entry points): checked before anything else, so that a bad block fails without a launch.
// fwd: a forward op (dsinks is a backward output).  On success *sinks / *dsinks are the pointers to use (NULL: none).
static int check_ext(const fa_ext_params* ext, const fa_params* p, bool bwd, const float** sinks, float** dsinks) {
    *sinks = nullptr;
    *dsinks = nullptr;
    if (!ext) return FA_OK;
    FA_CHECK(ext->struct_size >= sizeof(fa_ext_params), "fa_ext_params::struct_size %zu is smaller than this library's fa_ext_params (%zu)",
             ext->struct_size, sizeof(fa_ext_params));
    FA_CHECK(bwd || !ext->dsinks, "fa_ext_params::dsinks is a backward output: set it only for fa_bwd_ext / fa_varlen_bwd_ext");
    FA_CHECK(!ext->dsinks || ext->sinks, "fa_ext_params::dsinks needs fa_ext_params::sinks");
    if (!ext->sinks) return FA_OK;
    FA_CHECK(p, "params is NULL");
    FA_CHECK((reinterpret_cast<uintptr_t>(ext->sinks) & 3) == 0 && (reinterpret_cast<uintptr_t>(ext->dsinks) & 3) == 0,
             "attention sinks: sinks / dsinks must be 4-byte aligned fp32 arrays");
    if (p->dtype == FA_FP8_E4M3) return fail(FA_ERR_UNSUPPORTED, "attention sinks are not supported with fp8-e4m3 q/k/v");
    if (p->p_dropout > 0.f || p->dmask) return fail(FA_ERR_UNSUPPORTED, "attention sinks are not supported with dropout");
    *sinks = ext->sinks;
    *dsinks = ext->dsinks;
    return FA_OK;
}

static fa::KArgs make_args(const fa_params& p, int block_m) {
    fa::KArgs a;
    memset(&a, 0, sizeof(a));
    a.p = p;
    a.n_qblocks_total = (p.seqlen_q + block_m - 1) / block_m;
    // causal-like masks make late q-blocks heavier: pair block i with its mirror (equal work)
    a.pair_qblocks = ((p.is_causal || p.window_right >= 0) && p.window_left < 0 && a.n_qblocks_total >= 2) ? 1 : 0;
    a.n_qblocks = a.pair_qblocks ? (a.n_qblocks_total + 1) / 2 : a.n_qblocks_total;
    a.has_bias = (p.alibi_slopes != nullptr) || (p.softcap > 0.f);
    a.scale_log2e = p.softmax_scale * fa::kLog2e;
    a.rp_dropout = 1.0f;
    if (p.p_dropout > 0.f) {
        const float keep = 1.0f - p.p_dropout;
        const float t = keep * 4294967295.0f;            // fp32 on purpose (== 2^32 * keep)
        a.drop_thr = t >= 4294967295.0f ? 0xffffffffu : (uint32_t)t;
        a.rp_dropout = 1.0f / keep;
    }
    return a;
}

// Packed sequences on the flat work list of 128-row blocks (fa_common.h: decode_work_flat): no mirrored pairs
static void set_flat_qblocks(fa::KArgs& a) {
    a.flat_blocks = a.p.total_q / 128 + a.p.batch;
    a.pair_qblocks = 0;
    a.n_qblocks = a.n_qblocks_total;
}

extern "C" {

int fa_abi_version(void) { return FA_ABI_VERSION; }
size_t fa_params_size(void) { return sizeof(fa_params); }
size_t fa_tree_params_size(void) { return sizeof(fa_tree_params); }
size_t fa_merge_params_size(void) { return sizeof(fa_merge_params); }
size_t fa_rotary_params_size(void) { return sizeof(fa_rotary_params); }
size_t fa_kv_store_params_size(void) { return sizeof(fa_kv_store_params); }
size_t fa_kv_gather_params_size(void) { return sizeof(fa_kv_gather_params); }
size_t fa_rope_store_params_size(void) { return sizeof(fa_rope_store_params); }
size_t fa_qk_norm_rope_store_params_size(void) { return sizeof(fa_qk_norm_rope_store_params); }
size_t fa_qk_norm_rope_bwd_params_size(void) { return sizeof(fa_qk_norm_rope_bwd_params); }
size_t fa_add_norm_params_size(void) { return sizeof(fa_add_norm_params); }
size_t fa_add_norm_bwd_params_size(void) { return sizeof(fa_add_norm_bwd_params); }
size_t fa_cross_entropy_params_size(void) { return sizeof(fa_cross_entropy_params); }
size_t fa_cross_entropy_bwd_params_size(void) { return sizeof(fa_cross_entropy_bwd_params); }
size_t fa_sample_params_size(void) { return sizeof(fa_sample_params); }
size_t fa_spec_accept_params_size(void) { return sizeof(fa_spec_accept_params); }
size_t fa_spec_walk_params_size(void) { return sizeof(fa_spec_walk_params); }
size_t fa_act_mul_params_size(void) { return sizeof(fa_act_mul_params); }
size_t fa_act_mul_bwd_params_size(void) { return sizeof(fa_act_mul_bwd_params); }
size_t fa_quant_fp8_params_size(void) { return sizeof(fa_quant_fp8_params); }
size_t fa_add_norm_quant_params_size(void) { return sizeof(fa_add_norm_quant_params); }
size_t fa_act_mul_quant_params_size(void) { return sizeof(fa_act_mul_quant_params); }
size_t fa_moe_route_params_size(void) { return sizeof(fa_moe_route_params); }
size_t fa_moe_route_bwd_params_size(void) { return sizeof(fa_moe_route_bwd_params); }
size_t fa_moe_sort_params_size(void) { return sizeof(fa_moe_sort_params); }
size_t fa_moe_permute_params_size(void) { return sizeof(fa_moe_permute_params); }
size_t fa_moe_combine_params_size(void) { return sizeof(fa_moe_combine_params); }
size_t fa_moe_combine_bwd_params_size(void) { return sizeof(fa_moe_combine_bwd_params); }
size_t fa_moe_gemm_params_size(void) { return sizeof(fa_moe_gemm_params); }
size_t fa_moe_gemm_wgrad_params_size(void) { return sizeof(fa_moe_gemm_wgrad_params); }
const char* fa_last_error(void) { return g_last_error.c_str(); }
const char* fa_build_info(void) {
    return "libfa_mi355: gfx950 (CDNA4) hand-written HIP; mfma_f32_32x32x16_{bf16,f16}, mfma_scale_f32_32x32x64_f8f6f4 (fp8 q/k/v forward); "
           "head_dim {64,128,256}; "
           "ops fwd/bwd/varlen_fwd/varlen_bwd/fwd_kvcache";
}


// The varlen forward's routes to the decode kernels.  Both hand them paged K / V in the kv-cache op's layout - q [B, T_q, H, D]
// with batch stride T_q rows, LSE [H, B T_q] - and need the split-KV workspace: fa_fwd_workspace_bytes() reports it, and without
// it the general path runs as before.
//  * uniform decode (vLLM-style callers: every sequence brings the same few query tokens, lengths from seqused_k or
//    cu_seqlens_k): the decode kernels (GQA packing, split-KV) serve the whole call instead of fa_fwd_kernel's one workgroup per
//    sequence and head (B 1, H 32/8, 8 k context: 240 -> 32 us; tools/varlen_decode_probe.py);
//  * a MIXED batch (vLLM-style unified step: many sequences with one - or a few - query tokens next to a prefill chunk): the
//    host cannot see the lengths, but it can see that most sequences must be short ((total_q - max_seqlen_q) / (batch - 1) <=
//    64).  Then the decode kernels run over ALL sequences in varlen-q mode and keep the ones with 1 .. T query rows
//    (DecArgs::cu_q; the others' workgroups leave at once), and fa_fwd_kernel runs with KArgs::skip_short_q = T for the rest:
//    32 decode sequences + a 512-token chunk over 8 k contexts 792 -> ~350 us (tools/mixed_batch_probe.py).  T = 32 / G query
//    rows (at most 8): one 32-row block per kv-head.
enum class VarlenRoute { General, Decode, Mixed };

// the decode launch's params: T query rows per sequence at most (the class bound; rows per sequence come from cu_seqlens_q)
static fa_params varlen_decode_params(const fa_params& p, int T, bool uniform) {
    fa_params d = p;
    d.cache_seqlens = p.seqused_k;                       // NULL: cu_seqlens_k differences (dec_cache_len in fa_decode.hip)
    d.seqused_k = nullptr;
    d.seqlen_q = T;
    // cu_seqlens_q stays: the kernels run in varlen-q mode (DecArgs::cu_q, class bound T = seqlen_q) and take every
    // sequence's rows and row count from the device.  total_q == batch x max_seqlen_q does NOT prove cu_seqlens_q[-1] ==
    // total_q - q may carry padding rows behind the last sequence (graph-captured serving steps), and then sequence b is
    // not at row b T (round-3 advisor finding)
    d.q_batch_stride = 0; d.o_batch_stride = 0; d.lse_batch_stride = 0;
    d.k_new = d.v_new = nullptr; d.seqlen_new = 0;
    d.rotary_cos = d.rotary_sin = nullptr; d.rotary_dim = 0;
    d.cache_batch_idx = nullptr; d.cache_leftpad = nullptr;
    d.num_splits = 0;
    if (uniform && d.seqlen_q == 1 && !d.alibi_slopes) d.is_causal = 0;
    if (d.is_causal) d.window_right = 0;
    return d;
}

// d: the decode launch's params (Decode, Mixed)
static VarlenRoute varlen_route(const fa_params& p, fa_params& d) {
    if (!p.block_table || !p.cu_seqlens_q || !p.cu_seqlens_k || p.p_dropout > 0.f || p.dmask) return VarlenRoute::General;
    if ((p.kv_dtype != p.dtype && p.kv_dtype != FA_FP8_E4M3) || p.page_block_size <= 0 || p.page_block_size % 16 != 0)
        return VarlenRoute::General;
    if (p.batch > 0 && p.seqlen_q > 0 && p.total_q == (int64_t)p.batch * p.seqlen_q) {     // uniform T_q (host-checkable)
        d = varlen_decode_params(p, p.seqlen_q, true);
        return fa::decode_takes(d) ? VarlenRoute::Decode : VarlenRoute::General;
    }
    if (p.batch < 4 || p.nheads_k <= 0 || p.total_q >= (int64_t)p.batch * p.seqlen_q) return VarlenRoute::General;   // uniform: above
    const int G = p.nheads_q / p.nheads_k;
    int T = 32 / (G > 0 ? G : 1);
    T = T < 1 ? 1 : (T > 8 ? 8 : T);
    if (p.seqlen_q <= T) return VarlenRoute::General;                  // everything is short: the uniform route or the general kernel
    // (the other sequences average more than 64 rows: few of them can be decode steps.  A wrong yes costs one launch of
    //  workgroups that leave at once, ~10 us; a wrong no costs the decode sequences a 128-row tile and a full stream each)
    if ((p.total_q - p.seqlen_q) > (int64_t)(p.batch - 1) * 64) return VarlenRoute::General;
    d = varlen_decode_params(p, T, false);
    return fa::decode_takes(d) ? VarlenRoute::Mixed : VarlenRoute::General;
}

size_t fa_fwd_workspace_bytes(const fa_params* p) {
    fa_params d;
    if (!p) return 0;
    if (p->dtype == FA_FP8_E4M3) return 0;               // fp8 q: one kernel, no split, no decode route
    if (varlen_route(*p, d) != VarlenRoute::General) return fa::decode_workspace_bytes(d);
    if (!p->cu_seqlens_q && !p->cu_seqlens_k && !p->block_table && p->seqlen_q > 0 && p->seqlen_k > 0 && p->kv_dtype == p->dtype) {
        // fa_fwd: partial outputs of a key-split one-wave causal launch (the struct as fa_fwd will see it)
        fa_params q = *p;
        q.seqused_k = nullptr;
        normalize(q, false);
        return fa::fwd_split_workspace_bytes(make_args(q, 128));
    }
    return 0;
}
size_t fa_bwd_workspace_bytes(const fa_params* pp) {
    if (!pp) return 0;
    fa_params p = *pp;
    // the flags as fa_bwd / fa_varlen_bwd will see them (the split of small dK/dV launches depends on the mask's shape)
    if (p.seqlen_q > 0 && p.seqlen_k > 0) normalize(p, false);
    return fa::bwd_workspace_bytes(p, p.cu_seqlens_q && !varlen_grid_env());
}
size_t fa_fwd_kvcache_workspace_bytes(const fa_params* pp) {
    if (!pp) return 0;
    fa_params p = *pp;                                   // what fa_fwd_kvcache launches with (the decode code reads these fields)
    p.cu_seqlens_q = p.cu_seqlens_k = p.seqused_k = nullptr;
    return fa::decode_workspace_bytes(p);
}

int fa_fwd(const fa_params* pp, void* stream) { return fa_fwd_ext(pp, nullptr, stream); }

int fa_fwd_ext(const fa_params* pp, const fa_ext_params* ext, void* stream) {
    const float* sinks;
    float* dsinks;
    int rc = check_ext(ext, pp, false, &sinks, &dsinks);
    if (rc) return rc;
    if (!pp) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    fa_params p = *pp;
    p.cu_seqlens_q = p.cu_seqlens_k = p.seqused_k = nullptr;
    p.block_table = nullptr;
    rc = check_common(p, true, true);
    if (rc) return rc;
    const bool q8 = p.dtype == FA_FP8_E4M3;
    if (q8) {
        rc = check_fp8_q(p);
        if (rc) return rc;
    }
    FA_CHECK(p.kv_dtype == p.dtype, "k/v must have the same dtype as q");
    FA_CHECK(p.seqlen_q >= 0 && p.seqlen_k >= 0, "sequence lengths must be non-negative");
    if (p.seqlen_q == 0) return FA_OK;
    normalize(p, false);
    fa::KArgs a = make_args(p, 128);
    a.sinks = sinks;
    rc = q8 ? fa::launch_fwd_fp8(a, static_cast<hipStream_t>(stream)) : fa::launch_fwd(a, static_cast<hipStream_t>(stream));
    if (rc) return fail(FA_ERR_UNSUPPORTED, "no forward kernel for this configuration");
    return check_hip("fa_fwd launch");
}

int fa_varlen_fwd(const fa_params* pp, void* stream) { return fa_varlen_fwd_ext(pp, nullptr, stream); }

int fa_varlen_fwd_ext(const fa_params* pp, const fa_ext_params* ext, void* stream) {
    const float* sinks;
    float* dsinks;
    int rc = check_ext(ext, pp, false, &sinks, &dsinks);
    if (rc) return rc;
    if (!pp) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    fa_params p = *pp;
    rc = check_common(p, true, true);
    if (rc) return rc;
    if (p.dtype == FA_FP8_E4M3) {
        // fp8-e4m3 q, k, v (fa_fwd_fp8.hip): non-paged, flat work list
        rc = check_fp8_q(p);
        if (rc) return rc;
        FA_CHECK(p.cu_seqlens_q && p.cu_seqlens_k, "cu_seqlens_q and cu_seqlens_k are required");
        if (p.total_q == 0 || p.seqlen_q == 0) return FA_OK;
        normalize(p, false);
        fa::KArgs a = make_args(p, 128);
        a.seqlens_k = p.seqused_k;
        if (p.total_q > 0) set_flat_qblocks(a);
        rc = fa::launch_fwd_fp8(a, static_cast<hipStream_t>(stream));
        if (rc) return fail(FA_ERR_UNSUPPORTED, "no fp8 varlen forward kernel for this configuration");
        return check_hip("fa_varlen_fwd (fp8) launch");
    }
    // fp8-e4m3 K / V (this build's extension, as in fa_fwd_kvcache): paged caches, forward only, head dim 64 / 128
    if (p.kv_dtype == FA_FP8_E4M3) {
        FA_CHECK(p.block_table, "fp8 K/V through the varlen op: paged K/V (block_table) only");
        FA_CHECK((p.head_dim == 64 || p.head_dim == 128) && p.head_dim_v == 0, "fp8 K/V: head dimension 64 or 128");
        FA_CHECK(p.p_dropout == 0.f && !p.dmask, "fp8 K/V: no dropout");
    } else {
        FA_CHECK(p.kv_dtype == p.dtype, "k/v must have the same dtype as q (or fp8-e4m3 for paged K/V)");
    }
    FA_CHECK(p.cu_seqlens_q && p.cu_seqlens_k, "cu_seqlens_q and cu_seqlens_k are required");
    if (p.block_table) {
        FA_CHECK(p.page_block_size > 0, "page_block_size must be positive");
        FA_CHECK(p.page_block_size % 16 == 0, "Paged KV cache block size must be divisible by 16");
    }
    if (p.p_dropout > 0.f && p.block_table) return fail(FA_ERR_UNSUPPORTED, "dropout with paged K/V is not supported");
    if (p.total_q == 0 || p.seqlen_q == 0) return FA_OK;
    int skip_short = 0;
    fa_params d;
    const VarlenRoute route = varlen_route(p, d);
    if (route != VarlenRoute::General) {
        const size_t need = fa::decode_workspace_bytes(d);
        if (need == 0 || (d.workspace && d.workspace_bytes >= need)) {
            fa::KArgs ad = make_args(d, 128);
            ad.seqlens_k = d.cache_seqlens;
            ad.kv_mode = 1;
            ad.sinks = sinks;
            rc = fa::launch_decode(ad, static_cast<hipStream_t>(stream));
            if (route == VarlenRoute::Decode) {
                if (rc) return fail(FA_ERR_UNSUPPORTED, "no decode kernel for this varlen configuration");
                return check_hip("fa_varlen_fwd (decode kernels) launch");
            }
            if (rc) return fail(FA_ERR_UNSUPPORTED, "no decode kernel for the short sequences of this varlen batch");
            skip_short = d.seqlen_q;                 // the general kernel below leaves those sequences out
        }
    }
    normalize(p, false);
    fa::KArgs a = make_args(p, 128);
    a.seqlens_k = p.seqused_k;
    a.skip_short_q = skip_short;
    a.sinks = sinks;
    if (p.total_q > 0 && !varlen_grid_env()) set_flat_qblocks(a);
    rc = fa::launch_fwd(a, static_cast<hipStream_t>(stream));
    if (rc) return fail(FA_ERR_UNSUPPORTED, "no varlen forward kernel for this configuration");
    return check_hip("fa_varlen_fwd launch");
}

int fa_fwd_kvcache(const fa_params* pp, void* stream) { return fa_fwd_kvcache_ext(pp, nullptr, stream); }

int fa_fwd_kvcache_ext(const fa_params* pp, const fa_ext_params* ext, void* stream) {
    return fa_fwd_kvcache_tree(pp, ext, nullptr, stream);
}

// fa_tree_params (fa_fwd_kvcache_tree): the block itself, checked with the extension block before anything else.
// *on: a tree accompanies the call (mask != NULL)
static int check_tree_block(const fa_tree_params* tree, const fa_params* p, bool* on) {
    *on = false;
    const bool flag = p && (p->flags & FA_FLAG_TREE_MASK) != 0;
    if (tree) {
        FA_CHECK(tree->struct_size >= sizeof(fa_tree_params), "fa_tree_params::struct_size %zu is smaller than this library's fa_tree_params (%zu)",
                 tree->struct_size, sizeof(fa_tree_params));
        *on = tree->mask != nullptr;
    }
    FA_CHECK(!flag || *on, "FA_FLAG_TREE_MASK is set but no tree block (fa_tree_params::mask) accompanies the call");
    FA_CHECK(!*on || flag, "a tree block accompanies the call but FA_FLAG_TREE_MASK is not set in fa_params::flags "
                           "(fa_fwd_kvcache_workspace_bytes() needs it to answer for the decode route)");
    return FA_OK;
}

// the tree call's own argument checks (after the op's: p is normalised apart from the mask fields); all on the host
static int check_tree_call(const fa_tree_params& t, const fa_params& p) {
    FA_CHECK(p.seqlen_q >= 2 && p.seqlen_q <= 64, "tree mask: seqlen_q must be in [2, 64] (got %d)", p.seqlen_q);
    FA_CHECK(t.mask_words == (p.seqlen_q + 31) / 32, "tree mask: mask_words must be ceil(seqlen_q / 32) = %d (got %d)",
             (p.seqlen_q + 31) / 32, t.mask_words);
    FA_CHECK((reinterpret_cast<uintptr_t>(t.mask) & 3) == 0 && (reinterpret_cast<uintptr_t>(t.depths) & 3) == 0,
             "tree mask: mask and depths must be 4-byte aligned");
    FA_CHECK(t.mask_batch_stride >= 0 && t.depths_batch_stride >= 0, "tree mask: batch strides must be >= 0 (0 = shared by the batch)");
    FA_CHECK(p.seqlen_new == 0 || p.seqlen_new == p.seqlen_q, "tree mask: seqlen_new must be 0 or seqlen_q (the tree's nodes are the new tokens)");
    FA_CHECK(p.window_left < 0 && p.window_right < 0, "tree mask: window_size must be (-1, -1)");
    if (p.alibi_slopes) return fail(FA_ERR_UNSUPPORTED, "tree mask: ALiBi is not supported (its distance term needs tree positions)");
    FA_CHECK(p.rotary_dim <= 0 || t.depths, "tree mask: depths are required with rotary_cos / rotary_sin (node t sits at cache_seqlens + depths[t])");
    if (!fa::decode_applicable(p)) return fail(FA_ERR_UNSUPPORTED, "tree mask: no decode kernel for this head dimension / cache dtype");
    return FA_OK;
}

int fa_fwd_kvcache_tree(const fa_params* pp, const fa_ext_params* ext, const fa_tree_params* tree, void* stream) {
    const float* sinks;
    float* dsinks;
    int rc = check_ext(ext, pp, false, &sinks, &dsinks);
    if (rc) return rc;
    bool tree_on;
    rc = check_tree_block(tree, pp, &tree_on);
    if (rc) return rc;
    if (!pp) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    fa_params p = *pp;
    p.cu_seqlens_q = p.cu_seqlens_k = p.seqused_k = nullptr;
    p.flags &= ~FA_FLAG_TREE_MASK;                       // (this op's own bit: check_common rejects it for every other op)
    rc = check_common(p, true);
    if (rc) return rc;
    FA_CHECK(p.kv_dtype == p.dtype || p.kv_dtype == FA_FP8_E4M3, "kcache/vcache must match q dtype or be fp8-e4m3");
    FA_CHECK(p.p_dropout == 0.f, "kvcache attention has no dropout");
    const bool paged = p.block_table != nullptr;
    if (paged) {
        FA_CHECK(!p.cache_batch_idx, "Paged KVcache does not support cache_batch_idx");
        // (the reference wants multiples of 256, fused_mha_forward_kvcache.cu:488; here any multiple of 16 works - pages of
        //  64 tokens and more take the aligned fast paths, smaller ones the per-row lookups)
        FA_CHECK(p.page_block_size > 0 && p.page_block_size % 16 == 0,
                 "Paged KV cache block size must be divisible by 16");
    }
    if (p.k_new || p.v_new) {
        FA_CHECK(p.k_new && p.v_new, "If key is supplied, value must also be passed in");
        FA_CHECK(p.cache_seqlens, "If key is supplied, seqlens_k must also be passed in");
        FA_CHECK(p.seqlen_new > 0, "seqlen_new must be positive when k/v are supplied");
        FA_CHECK(p.seqlen_new <= p.seqlen_k && p.seqlen_q <= p.seqlen_k,
                 "new keys / queries do not fit the cache (fused_mha_forward_kvcache.cu: T_Q <= max_seqlen_k)");
    } else {
        p.seqlen_new = 0;
    }
    if (p.rotary_dim > 0) {
        FA_CHECK(p.k_new, "If rotary cos/sin are provided, new key / value to be appended to KV cache must also be provided");
        FA_CHECK(p.rotary_cos && p.rotary_sin, "rotary_cos and rotary_sin must both be given");
        FA_CHECK(p.rotary_dim <= (p.head_dim_v > 0 ? p.head_dim_v : p.head_dim), "rotary_dim must be <= headdim");
        FA_CHECK(p.rotary_dim % 16 == 0, "rotary_dim must be divisible by 16");
        // every position the kernels can touch is < the cache capacity (append and rotation are range-guarded)
        FA_CHECK(p.seqlen_ro >= p.seqlen_k, "rotary_cos / rotary_sin must cover the cache capacity (seqlen_ro >= seqlen_k)");
    }
    if (p.num_splits < 0) return fail(FA_ERR_INVALID_ARGUMENT, "num_splits must be >= 0");
    if (tree_on) {
        // the mask replaces the causal rule (windows are checked as the caller gave them: causal alone sets none)
        p.is_causal = 0;
        rc = check_tree_call(*tree, p);
        if (rc) return rc;
        p.flags |= FA_FLAG_TREE_MASK;                    // decode_takes(): every tree call runs on the decode kernels
    }
    // reference: fused_mha_forward_kvcache.cu:465-472
    normalize(p, true);
    if (p.softcap > 0.f) {
        FA_CHECK(p.window_left < 0 && p.window_right < 0, "Softcap + window not supported");
        FA_CHECK(!p.alibi_slopes, "Softcap + ALiBi not supported");
    }
    if (p.seqlen_q == 0) return FA_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    fa::KArgs a = make_args(p, 128);
    a.seqlens_k = p.cache_seqlens;
    a.seqlen_k_add = p.seqlen_new;
    a.kv_batch_idx = p.cache_batch_idx;
    a.leftpad_k = p.cache_leftpad;
    a.kv_mode = 1;
    a.sinks = sinks;
    rc = fa::launch_decode(a, s, tree_on ? tree : nullptr);
    if (rc == -2) return fail(FA_ERR_UNSUPPORTED, "no kvcache kernel for this configuration (fp8 caches: head_dim 64 or 128)");
    if (rc == -1) return fail(FA_ERR_INVALID_ARGUMENT, "workspace too small: query fa_fwd_kvcache_workspace_bytes()");
    if (rc) return rc;
    return check_hip("fa_fwd_kvcache launch");
}

// The sinks' gradient (fa_bwd_ext / fa_varlen_bwd_ext): after launch_bwd on the same stream, when softmax_d is final
// whichever kernel wrote it; zeros when there are no query rows.
static int dsinks_launch(const fa::KArgs& a, const float* sinks, float* dsinks, bool no_rows, hipStream_t s) {
    if (!dsinks) return FA_OK;
    if (no_rows) {
        if (hipMemsetAsync(dsinks, 0, (size_t)a.p.nheads_q * sizeof(float), s) != hipSuccess)
            return fail(FA_ERR_LAUNCH, "hipMemsetAsync(dsinks) failed");
        return FA_OK;
    }
    fa::KArgs a2 = a;
    a2.sinks = sinks;
    fa::launch_bwd_dsinks(a2, dsinks, s);
    return check_hip("dsinks launch");
}

int fa_bwd(const fa_params* pp, void* stream) { return fa_bwd_ext(pp, nullptr, stream); }

int fa_bwd_ext(const fa_params* pp, const fa_ext_params* ext, void* stream) {
    const float* sinks;
    float* dsinks;
    int rc = check_ext(ext, pp, true, &sinks, &dsinks);
    if (rc) return rc;
    if (!pp) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    fa_params p = *pp;
    p.cu_seqlens_q = p.cu_seqlens_k = p.seqused_k = nullptr;
    p.block_table = nullptr;
    rc = check_common(p, true);
    if (rc) return rc;
    FA_CHECK(p.dout && p.softmax_d, "dout and softmax_d must not be NULL");
    FA_CHECK((p.dk == nullptr) == (p.dv == nullptr), "dk and dv must be given (or left NULL) together");
    FA_CHECK(p.kv_dtype == p.dtype, "k/v must have the same dtype as q");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.seqlen_q == 0 && p.seqlen_k == 0) return dsinks_launch(make_args(p, 128), sinks, dsinks, true, s);
    normalize(p, false);
    fa::KArgs a = make_args(p, 128);
    rc = fa::launch_bwd(a, s);
    if (rc == -2) return fail(FA_ERR_UNSUPPORTED, "no backward kernel for this configuration");
    if (rc) return rc;
    rc = check_hip("fa_bwd launch");
    if (rc) return rc;
    return dsinks_launch(a, sinks, dsinks, p.seqlen_q == 0, s);
}

int fa_varlen_bwd(const fa_params* pp, void* stream) { return fa_varlen_bwd_ext(pp, nullptr, stream); }

int fa_varlen_bwd_ext(const fa_params* pp, const fa_ext_params* ext, void* stream) {
    const float* sinks;
    float* dsinks;
    int rc = check_ext(ext, pp, true, &sinks, &dsinks);
    if (rc) return rc;
    if (!pp) return fail(FA_ERR_INVALID_ARGUMENT, "params is NULL");
    fa_params p = *pp;
    p.block_table = nullptr;
    rc = check_common(p, true);
    if (rc) return rc;
    FA_CHECK(p.dout && p.softmax_d, "dout and softmax_d must not be NULL");
    FA_CHECK((p.dk == nullptr) == (p.dv == nullptr), "dk and dv must be given (or left NULL) together");
    FA_CHECK(p.cu_seqlens_q && p.cu_seqlens_k, "cu_seqlens_q and cu_seqlens_k are required");
    FA_CHECK(p.kv_dtype == p.dtype, "k/v must have the same dtype as q");
    if (p.total_q == 0) {
        // no query rows: nothing flows into K / V - the gradients are zeros, written here (not left to the caller)
        const int64_t rows = p.total_k;
        const size_t width = (size_t)(p.head_dim_v > 0 ? p.head_dim_v : p.head_dim) * 2;
        hipStream_t s = static_cast<hipStream_t>(stream);
        for (int h = 0; h < p.nheads_k && rows > 0 && p.dk; ++h) {
            if (hipMemset2DAsync(reinterpret_cast<uint16_t*>(p.dk) + (int64_t)h * p.dk_head_stride, (size_t)p.dk_row_stride * 2, 0, width, (size_t)rows, s) != hipSuccess ||
                hipMemset2DAsync(reinterpret_cast<uint16_t*>(p.dv) + (int64_t)h * p.dv_head_stride, (size_t)p.dv_row_stride * 2, 0, width, (size_t)rows, s) != hipSuccess)
                return fail(FA_ERR_LAUNCH, "hipMemset2DAsync(dk / dv) failed");
        }
        return dsinks_launch(make_args(p, 128), sinks, dsinks, true, s);
    }
    normalize(p, false);
    fa::KArgs a = make_args(p, 128);
    if (!varlen_grid_env()) set_flat_qblocks(a);
    rc = fa::launch_bwd(a, static_cast<hipStream_t>(stream));
    if (rc == -2) return fail(FA_ERR_UNSUPPORTED, "no varlen backward kernel for this configuration");
    if (rc) return rc;
    rc = check_hip("fa_varlen_bwd launch");
    if (rc) return rc;
    return dsinks_launch(a, sinks, dsinks, false, static_cast<hipStream_t>(stream));
}

int fa_gather_rows(const void* src, const int64_t* indices, void* dst, int64_t n_idx, int64_t row_bytes,
                   int64_t src_row_stride_bytes, int64_t n_src_rows, void* stream) {
    FA_CHECK(n_idx >= 0 && row_bytes >= 0 && n_src_rows >= 0, "sizes must be non-negative");
    if (n_idx == 0 || row_bytes == 0) return FA_OK;
    FA_CHECK(src && indices && dst, "src, indices and dst must not be NULL");
    FA_CHECK(row_bytes % 16 == 0 && src_row_stride_bytes % 16 == 0 && src_row_stride_bytes >= row_bytes,
             "row_bytes and src_row_stride_bytes must be multiples of 16 (stride >= row)");
    FA_CHECK(((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0), "src and dst must be 16-byte aligned");
    fa::launch_gather_rows(src, indices, dst, n_idx, row_bytes, src_row_stride_bytes, n_src_rows, static_cast<hipStream_t>(stream));
    return check_hip("fa_gather_rows launch");
}

int fa_scatter_rows(const void* src, const int64_t* indices, void* dst, int64_t n_idx, int64_t n_dst_rows,
                    int64_t row_bytes, int sorted_unique, void* stream) {
    FA_CHECK(n_idx >= 0 && row_bytes >= 0 && n_dst_rows >= 0, "sizes must be non-negative");
    if (n_dst_rows == 0 || row_bytes == 0) return FA_OK;
    FA_CHECK(dst && (n_idx == 0 || (src && indices)), "src, indices and dst must not be NULL");
    FA_CHECK(row_bytes % 16 == 0, "row_bytes must be a multiple of 16");
    FA_CHECK(((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0), "src and dst must be 16-byte aligned");
    if (fa::launch_scatter_rows(src, indices, dst, n_idx, n_dst_rows, row_bytes, sorted_unique, static_cast<hipStream_t>(stream)))
        return fail(FA_ERR_INVALID_ARGUMENT, "hipMemsetAsync failed");
    return check_hip("fa_scatter_rows launch");
}

int fa_merge_states(const fa_merge_params* m, void* stream) {
    FA_CHECK(m, "fa_merge_params must not be NULL");
    FA_CHECK(m->struct_size >= sizeof(fa_merge_params), "fa_merge_params::struct_size %zu is smaller than this library's %zu",
             m->struct_size, sizeof(fa_merge_params));
    FA_CHECK(m->n_parts >= 2 && m->n_parts <= FA_MERGE_MAX_PARTS, "n_parts must be 2 .. %d, got %d", FA_MERGE_MAX_PARTS, m->n_parts);
    FA_CHECK(m->dtype == FA_FP16 || m->dtype == FA_BF16, "merge dtype must be fp16 or bf16");
    FA_CHECK(m->head_dim > 0 && m->head_dim % 8 == 0 && m->head_dim <= 256, "merge head_dim must be a multiple of 8 and <= 256, got %d",
             m->head_dim);
    FA_CHECK(m->batch >= 0 && m->seqlen >= 0 && m->nheads >= 0, "merge sizes must be non-negative");
    for (int s = 0; s <= m->n_parts; ++s) {
        const bool is_out = s == m->n_parts;
        const fa_merge_state& t = is_out ? m->out : m->parts[s];
        FA_CHECK(t.o && t.lse, "merge %s %d: o and lse must not be NULL", is_out ? "output" : "part", is_out ? 0 : s);
        FA_CHECK((uintptr_t)t.lse % 4 == 0, "merge %s %d: lse must be 4-byte aligned", is_out ? "output" : "part", is_out ? 0 : s);
        if (!is_out)
            FA_CHECK(t.o != m->out.o && t.lse != m->out.lse, "merge output must not alias part %d (no in-place merge)", s);
    }
    FA_CHECK(fa::merge_vec_width(*m) != 0, "merge: every o base address and stride must be a multiple of 8 bytes");
    if (m->batch == 0 || m->seqlen == 0 || m->nheads == 0) return FA_OK;
    // (one lane per 8-byte piece at the least: the 1-D grid of 256-lane workgroups must fit 31 bits)
    if ((double)m->batch * m->seqlen * m->nheads * (m->head_dim / 4) >= 256.0 * 2147483647.0)
        return fail(FA_ERR_UNSUPPORTED, "merge: batch x seqlen x nheads x head_dim is too large for one launch");
    fa::launch_merge_states(*m, static_cast<hipStream_t>(stream));
    return check_hip("fa_merge_states launch");
}

}  // extern "C"

// ---- The row ops around attention (fa_rotary .. fa_act_mul_quant): one argument-checking layer, then the entry points. ----
// Every helper takes `op`, the name its messages begin with, and is parameterised by data alone: pointers, sizes and which fields
// a block has.  A rule that only one op has stays in that op's own function.

#define FA_TRY(expr)                         \
    do {                                     \
        const int rc_ = (expr);              \
        if (rc_ != FA_OK) return rc_;        \
    } while (0)

static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// the head of every struct-taking entry point: the block is there and not smaller than this library's
template <typename P>
static int check_header(const P* p, const char* type) {
    FA_CHECK(p, "%s must not be NULL", type);
    FA_CHECK(p->struct_size >= sizeof(P), "%s::struct_size %zu is smaller than this library's %zu", type, p->struct_size, sizeof(P));
    return FA_OK;
}

// `what` names the tensors in the message: "k / v dtype", "dtype", ...
static int check_io_dtype(const char* op, int dtype, const char* what) {
    FA_CHECK(dtype == FA_FP16 || dtype == FA_BF16, "%s: %s must be fp16 or bf16", op, what);
    return FA_OK;
}

static int check_cache_dtype(const char* op, int cache_dtype, int dtype) {
    FA_CHECK(cache_dtype == dtype || cache_dtype == FA_FP8_E4M3, "%s: the cache dtype must be the k / v dtype or fp8-e4m3", op);
    return FA_OK;
}

// P: a block with k_cache / v_cache and their kc_* / vc_* strides
template <typename P>
static int check_cache_align(const char* op, const P& s, bool kv8) {
    const uintptr_t cal = kv8 ? 7 : 15;                   // bytes; strides are in elements of 1 / 2 bytes
    const int64_t sal = 7;
    FA_CHECK(((addr(s.k_cache) | addr(s.v_cache)) & cal) == 0 &&
             ((s.kc_batch_stride | s.kc_row_stride | s.kc_head_stride | s.vc_batch_stride | s.vc_row_stride | s.vc_head_stride) & sal) == 0,
             "%s: cache base addresses and strides must be multiples of %d bytes", op, kv8 ? 8 : 16);
    return FA_OK;
}

// checked for every cache type, used by fp8 caches; normalises 0 to 1.0
static int check_descales(const char* op, float& k_descale, float& v_descale) {
    float* ds[2] = {&k_descale, &v_descale};
    for (float* d : ds) {
        FA_CHECK(*d >= 0.f && *d <= 3.402823466e38f, "%s: k / v descales must be finite and >= 0 (0 = 1.0)", op);
        if (*d == 0.f) *d = 1.0f;
    }
    return FA_OK;
}

// The rotary-table group of a block with positions / rotary_cos / rotary_sin / rotary_dim / seqlen_ro / head_dim, in the three
// places where the per-token ops look at it (between them come the op's own sizes, which the later rules rely on).
// 1. which pointers are there.  no_rope_ok: seqlen_ro == 0 means "no rotation" - positions and the tables may be NULL then and
//    rotary_dim is not read (the block is normalised: all four cleared); otherwise all three are required, and so is k.
//    Returns *no_rope.
template <typename P>
static int check_rope_tables(const char* op, P& s, bool no_rope_ok, bool* no_rope) {
    *no_rope = no_rope_ok && s.seqlen_ro == 0;
    if (*no_rope) {
        s.positions = nullptr; s.rotary_cos = s.rotary_sin = nullptr; s.rotary_dim = 0;
    } else if (no_rope_ok) {
        FA_CHECK(s.seqlen_ro < 0 || (s.positions && s.rotary_cos && s.rotary_sin),             // (< 0: rejected with the op's sizes)
                 "%s: positions, rotary_cos and rotary_sin may be NULL only where seqlen_ro == 0", op);
    } else {
        FA_CHECK(s.k && s.positions && s.rotary_cos && s.rotary_sin, "%s: k, positions, rotary_cos and rotary_sin must not be NULL", op);
    }
    return FA_OK;
}
// 2. rotary_dim against the kernels' 16-column pieces and against head_dim
template <typename P>
static int check_rope_dims(const char* op, const P& s, bool no_rope) {
    if (!no_rope) FA_CHECK(s.rotary_dim > 0 && s.rotary_dim % 16 == 0, "%s: rotary_dim must be positive and divisible by 16, got %d", op, s.rotary_dim);
    FA_CHECK(s.rotary_dim <= s.head_dim, "%s: rotary_dim must be <= head_dim (%d > %d)", op, s.rotary_dim, s.head_dim);
    return FA_OK;
}
// 3. where the tables lie
template <typename P>
static int check_rope_align(const char* op, const P& s) {
    FA_CHECK(((addr(s.rotary_cos) | addr(s.rotary_sin)) & 15) == 0, "%s: rotary_cos / rotary_sin must be 16-byte aligned", op);
    return FA_OK;
}

// The norm scalars.  io: how the message names the 16-bit dtype ("q / k dtype", "io dtype")
static int check_weight_dtype(const char* op, int weight_dtype, int dtype, const char* io) {
    FA_CHECK(weight_dtype == FA_FP32 || (weight_dtype == dtype && (dtype == FA_FP16 || dtype == FA_BF16)),
             "%s: weight_dtype must be the %s or fp32", op, io);
    return FA_OK;
}
static int check_norm_scalars(const char* op, float eps, float weight_offset) {
    FA_CHECK(eps >= 0.f && eps <= 3.402823466e38f, "%s: eps must be finite and >= 0", op);
    FA_CHECK(weight_offset >= -3.402823466e38f && weight_offset <= 3.402823466e38f, "%s: weight_offset must be finite", op);
    return FA_OK;
}

// bytes from the first to one past the last element of a [blocks, rows, heads, d] tensor (sizes > 0, strides >= 0, in elements)
static uint64_t span_bytes(int64_t blocks, int64_t bs, int64_t rows, int64_t rs, int64_t heads, int64_t hs, int64_t d, int esize) {
    return (uint64_t)((blocks - 1) * bs + (rows - 1) * rs + (heads - 1) * hs + d) * (uint64_t)esize;
}

// What the overlap rules look at (bytes): `rows` rows of row_bytes each, row_stride apart; a NULL pointer or no element: empty.
// note: the hint a message ends with where both the output and the input of a pair carry one (the input's is printed)
struct View { const char* name; uint64_t at, row_stride, row_bytes, bytes; const char* note; };
// rows of `row_elems` elements (a head-strided row: (heads - 1) * head_stride + head_dim), the row stride in elements
static View view_rows(const char* name, const void* p, int64_t rows, int64_t rs, int64_t row_elems, int esize, const char* note = nullptr) {
    View v = {name, (uint64_t)addr(p), (uint64_t)rs * esize, 0, 0, note};
    if (p && rows > 0 && row_elems > 0) {
        v.row_bytes = (uint64_t)row_elems * esize;
        v.bytes = (uint64_t)(rows - 1) * v.row_stride + v.row_bytes;
    }
    return v;
}
// one address range: the rule for it is the plain range test
static View view_flat(const char* name, const void* p, uint64_t bytes, const char* note = nullptr) {
    return View{name, (uint64_t)addr(p), 0, p ? bytes : 0, p ? bytes : 0, note};
}
// no common element: disjoint address ranges, or the heads / column ranges of one packed buffer - the same row stride, and within
// a row the one view ends before the other begins
static bool views_disjoint(const View& a, const View& b) {
    if (!a.bytes || !b.bytes || a.at >= b.at + b.bytes || b.at >= a.at + a.bytes) return true;
    const View& lo = a.at <= b.at ? a : b;
    const View& hi = a.at <= b.at ? b : a;
    const uint64_t delta = hi.at - lo.at;
    return a.row_stride == b.row_stride && delta < lo.row_stride && lo.row_bytes <= delta && delta + hi.row_bytes <= lo.row_stride;
}
// every output against every input and - among_outs - against the later outputs; exempt[k] = {output, input}, k < n_ex: the exact
// in-place pairs, which the caller guarantees
static int check_overlaps(const char* op, const View* out, int n_out, const View* in, int n_in, bool among_outs,
                          const int (*exempt)[2] = nullptr, int n_ex = 0) {
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i) {
            bool ex = false;
            for (int k = 0; k < n_ex; ++k) ex = ex || (exempt[k][0] == o && exempt[k][1] == i);
            FA_CHECK(ex || views_disjoint(out[o], in[i]), "%s: %s overlaps %s%s", op, out[o].name, in[i].name,
                     out[o].note && in[i].note ? in[i].note : "");
        }
        for (int p = o + 1; among_outs && p < n_out; ++p)
            FA_CHECK(views_disjoint(out[o], out[p]), "%s: %s overlaps %s", op, out[o].name, out[p].name);
    }
    return FA_OK;
}

static int rotary_check(const fa_rotary_params& r, bool* empty) {
    FA_CHECK(r.x && r.out && r.cos && r.sin, "rotary: x, out, cos and sin must not be NULL");
    FA_CHECK(r.dtype == FA_FP16 || r.dtype == FA_BF16, "rotary dtype must be fp16 or bf16");
    FA_CHECK(r.batch >= 0 && r.seqlen >= 0 && r.nheads >= 0 && r.head_dim >= 0 && r.seqlen_ro >= 0 && r.total_rows >= 0 &&
             r.seqlen_offset >= 0, "rotary sizes and seqlen_offset must be non-negative");
    FA_CHECK(r.rotary_dim > 0 && r.rotary_dim % 2 == 0, "rotary_dim must be positive and even, got %d", r.rotary_dim);
    FA_CHECK(r.rotary_dim <= r.head_dim, "rotary_dim must be <= head_dim (%d > %d)", r.rotary_dim, r.head_dim);
    FA_CHECK(r.x_batch_stride >= 0 && r.x_row_stride >= 0 && r.x_head_stride >= 0 && r.o_batch_stride >= 0 &&
             r.o_row_stride >= 0 && r.o_head_stride >= 0, "rotary strides must be non-negative");
    FA_CHECK(addr(r.x) % 2 == 0 && addr(r.out) % 2 == 0, "rotary: x and out must be 2-byte aligned");
    const uintptr_t cs_al = r.cos_sin_fp32 ? 4 : 2;
    FA_CHECK(addr(r.cos) % cs_al == 0 && addr(r.sin) % cs_al == 0,
             "rotary: cos / sin must be aligned to their element size (%d bytes)", (int)cs_al);
    FA_CHECK(addr(r.seqlen_offsets) % 4 == 0 && addr(r.cu_seqlens) % 4 == 0,
             "rotary: seqlen_offsets and cu_seqlens must be 4-byte aligned int32 arrays");
    if ((int64_t)r.nheads * r.head_dim > ((int64_t)1 << 24))
        return fail(FA_ERR_UNSUPPORTED, "rotary: nheads x head_dim is too large for one launch");
    *empty = r.batch == 0 || r.nheads == 0 || (r.cu_seqlens ? r.total_rows == 0 : r.seqlen == 0);
    if (*empty) return FA_OK;
    if (r.x == r.out) {
        FA_CHECK(r.x_row_stride == r.o_row_stride && r.x_head_stride == r.o_head_stride &&
                 (r.cu_seqlens || r.x_batch_stride == r.o_batch_stride),
                 "rotary: out shares x's base address but not its strides (in place needs both equal)");
        return FA_OK;
    }
    // x / out as fa_rotary addresses them: one address range each
    const char* note = " without being x itself (in place: the same base address and strides)";
    const int64_t blocks = r.cu_seqlens ? 1 : r.batch, rows = r.cu_seqlens ? r.total_rows : r.seqlen;
    const View x = view_flat("x", r.x, span_bytes(blocks, r.x_batch_stride, rows, r.x_row_stride, r.nheads, r.x_head_stride, r.head_dim, 2), note);
    const View out = view_flat("out", r.out, span_bytes(blocks, r.o_batch_stride, rows, r.o_row_stride, r.nheads, r.o_head_stride, r.head_dim, 2), note);
    return check_overlaps("rotary", &out, 1, &x, 1, false);
}

// What fa_kv_store and fa_kv_gather share: a packed k / v pair, a cache pair and the two addressing modes.  P: either block.
// seq_base / seq_base_name: the op's own per-sequence int32 array of sequence mode (cache_seqlens, seq_offsets); more_sizes_ok:
// the op's further sizes are non-negative.  Normalises the descales; *seq_mode: cu_seqlens addressing.
template <typename P>
static int kv_rows_check(const char* op, P& s, const void* seq_base, const char* seq_base_name, bool more_sizes_ok, bool* seq_mode) {
    FA_CHECK(s.k && s.v && s.k_cache && s.v_cache, "%s: k, v, k_cache and v_cache must not be NULL", op);
    FA_TRY(check_io_dtype(op, s.dtype, "k / v dtype"));
    FA_TRY(check_cache_dtype(op, s.cache_dtype, s.dtype));
    const bool slot_mode = s.slot_mapping != nullptr;
    *seq_mode = s.cu_seqlens != nullptr;
    FA_CHECK(slot_mode != *seq_mode, "%s: exactly one addressing mode - slot_mapping, or cu_seqlens (%s given)", op, slot_mode ? "both" : "neither");
    FA_CHECK(!(s.block_table && s.cache_batch_idx), "%s: block_table and cache_batch_idx exclude each other (paged caches have no cache_batch_idx)", op);
    FA_CHECK(s.total_rows >= 0 && s.nheads >= 0 && s.head_dim >= 0 && s.num_blocks >= 0 && s.batch >= 0 && s.max_blocks >= 0 &&
             more_sizes_ok, "%s sizes must be non-negative", op);
    FA_CHECK(s.head_dim % 8 == 0 && s.head_dim <= 256, "%s head_dim must be a multiple of 8 and <= 256, got %d", op, s.head_dim);
    FA_CHECK(s.page_block_size > 0, "%s: page_block_size must be positive (a contiguous cache: S_max)", op);
    FA_CHECK(s.k_row_stride >= 0 && s.k_head_stride >= 0 && s.v_row_stride >= 0 && s.v_head_stride >= 0 && s.kc_batch_stride >= 0 &&
             s.kc_row_stride >= 0 && s.kc_head_stride >= 0 && s.vc_batch_stride >= 0 && s.vc_row_stride >= 0 &&
             s.vc_head_stride >= 0 && s.block_table_batch_stride >= 0, "%s strides must be non-negative", op);
    if (slot_mode) {
        FA_CHECK(!seq_base && !s.block_table && !s.cache_batch_idx,
                 "%s: slot mode takes no %s, block_table or cache_batch_idx (the slot is the whole address)", op, seq_base_name);
    } else {
        if (s.paged) FA_CHECK(s.block_table, "%s: sequence mode on a paged cache needs a block_table", op);
        else         FA_CHECK(!s.block_table, "%s: a block_table needs paged != 0", op);
        FA_CHECK(s.paged || s.cache_batch_idx || s.batch <= s.num_blocks,
                 "%s: the cache has %d batch slots for %d sequences (pass cache_batch_idx)", op, s.num_blocks, s.batch);
        FA_CHECK(addr(s.cu_seqlens) % 4 == 0 && addr(seq_base) % 4 == 0 && addr(s.block_table) % 4 == 0 && addr(s.cache_batch_idx) % 4 == 0,
                 "%s: cu_seqlens, %s, block_table and cache_batch_idx must be 4-byte aligned int32 arrays", op, seq_base_name);
    }
    return FA_OK;
}
// ... and, behind the op's own slot-mode rules, where the tensors lie and the descales
template <typename P>
static int kv_rows_check_layout(const char* op, P& s) {
    if (s.slot_mapping) FA_CHECK(addr(s.slot_mapping) % 8 == 0, "%s: slot_mapping must be an 8-byte aligned int64 array", op);
    FA_CHECK(((addr(s.k) | addr(s.v)) & 15) == 0 && ((s.k_row_stride | s.k_head_stride | s.v_row_stride | s.v_head_stride) & 7) == 0,
             "%s: k / v base addresses and strides must be multiples of 16 bytes", op);
    FA_TRY(check_cache_align(op, s, s.cache_dtype == FA_FP8_E4M3));
    return check_descales(op, s.k_descale, s.v_descale);
}

// fa_kv_store's argument rules; normalises the block.  *empty: nothing to launch
static int kv_store_check(fa_kv_store_params& s, bool* empty) {
    const char* op = "kv_store";
    bool seq_mode;
    FA_TRY(kv_rows_check(op, s, s.cache_seqlens, "cache_seqlens", s.seqlen_ro >= 0 && s.rotary_dim >= 0, &seq_mode));
    if (!seq_mode)
        FA_CHECK(s.rotary_dim == 0 && !s.rotary_cos && !s.rotary_sin,
                 "kv_store: rotary needs sequence mode (a slot carries no position); rotate with fa_rotary first");
    FA_TRY(kv_rows_check_layout(op, s));
    if (s.rotary_dim > 0 || s.rotary_cos || s.rotary_sin) {
        // fa_fwd_kvcache's constraints (the tables need not cover the capacity here: a position outside them is stored unrotated)
        FA_CHECK(s.rotary_cos && s.rotary_sin, "rotary_cos and rotary_sin must both be given");
        FA_CHECK(s.rotary_dim > 0, "kv_store: rotary_cos / rotary_sin need rotary_dim > 0");
        FA_CHECK(s.rotary_dim <= s.head_dim, "rotary_dim must be <= headdim");
        FA_CHECK(s.rotary_dim % 16 == 0, "rotary_dim must be divisible by 16");
        FA_TRY(check_rope_align(op, s));
    }
    if ((int64_t)s.nheads * s.head_dim > ((int64_t)1 << 24))
        return fail(FA_ERR_UNSUPPORTED, "kv_store: nheads x head_dim is too large for one launch");
    *empty = s.total_rows == 0 || s.nheads == 0 || s.head_dim == 0 || (seq_mode && s.batch == 0);
    return FA_OK;
}

// fa_kv_gather's argument rules; normalises the block.  *empty: nothing to launch
static int kv_gather_check(fa_kv_gather_params& s, bool* empty) {
    const char* op = "kv_gather";
    bool seq_mode;
    FA_TRY(kv_rows_check(op, s, s.seq_offsets, "seq_offsets", true, &seq_mode));
    FA_TRY(kv_rows_check_layout(op, s));
    if ((int64_t)s.nheads * s.head_dim > ((int64_t)1 << 24))
        return fail(FA_ERR_UNSUPPORTED, "kv_gather: nheads x head_dim is too large for one launch");
    *empty = s.total_rows == 0 || s.nheads == 0 || s.head_dim == 0;
    if (*empty || s.num_blocks == 0) return FA_OK;
    // the output must not lie inside what is read: the rows are written while other workgroups still read the cache
    const int csize = s.cache_dtype == FA_FP8_E4M3 ? 1 : 2;
    const char* note = " (gather into a separate buffer)";
    const View in[] = {
        view_flat("k_cache", s.k_cache, span_bytes(s.num_blocks, s.kc_batch_stride, s.page_block_size, s.kc_row_stride, s.nheads, s.kc_head_stride, s.head_dim, csize), note),
        view_flat("v_cache", s.v_cache, span_bytes(s.num_blocks, s.vc_batch_stride, s.page_block_size, s.vc_row_stride, s.nheads, s.vc_head_stride, s.head_dim, csize), note),
    };
    const View out[] = {
        view_flat("k", s.k, span_bytes(1, 0, s.total_rows, s.k_row_stride, s.nheads, s.k_head_stride, s.head_dim, 2), note),
        view_flat("v", s.v, span_bytes(1, 0, s.total_rows, s.v_row_stride, s.nheads, s.v_head_stride, s.head_dim, 2), note),
    };
    return check_overlaps(op, out, 2, in, 2, false);
}

// The argument rules that fa_rope_store and fa_qk_norm_rope_store share.  P: either block (the second begins with the fields of
// the first).  no_rope_ok: see check_rope_tables.  extra: further read-only views that an out-of-place output must not overlap.
// Normalises the block (descales of 0 -> 1.0, nheads_q = 0 without q); *empty: nothing to launch.
template <typename P>
static int rope_store_check(P& s, const char* op, bool no_rope_ok, const View* extra, int n_extra, bool* empty) {
    *empty = false;
    if (no_rope_ok) FA_CHECK(s.k, "%s: k must not be NULL", op);
    bool no_rope;
    FA_TRY(check_rope_tables(op, s, no_rope_ok, &no_rope));
    FA_CHECK((s.q != nullptr) == (s.q_out != nullptr), "%s: q and q_out go together (%s given)", op, s.q ? "q without q_out" : "q_out without q");
    FA_CHECK((s.k_cache != nullptr) == (s.v_cache != nullptr), "%s: k_cache and v_cache go together (both, or neither: rotate only)", op);
    const bool cached = s.k_cache != nullptr;
    if (cached) {
        FA_CHECK(s.v && s.slot_mapping, "%s: caches need v and slot_mapping", op);
    } else {
        FA_CHECK(!s.v && !s.slot_mapping, "%s: v and slot_mapping need caches (the rotate-only form takes neither)", op);
        FA_CHECK(s.q || s.k_out, "%s: the rotate-only form needs q or k_out (nothing would be written)", op);
    }
    FA_TRY(check_io_dtype(op, s.dtype, "q / k / v dtype"));
    if (cached) FA_TRY(check_cache_dtype(op, s.cache_dtype, s.dtype));
    FA_CHECK(s.total_rows >= 0 && s.nheads_q >= 0 && s.nheads_k >= 0 && s.head_dim >= 0 && s.seqlen_ro >= 0 && s.num_blocks >= 0,
             "%s sizes must be non-negative", op);
    FA_CHECK(s.head_dim % 8 == 0 && s.head_dim <= 256, "%s head_dim must be a multiple of 8 and <= 256, got %d", op, s.head_dim);
    FA_TRY(check_rope_dims(op, s, no_rope));
    FA_CHECK(s.q_row_stride >= 0 && s.q_head_stride >= 0 && s.k_row_stride >= 0 && s.k_head_stride >= 0 && s.v_row_stride >= 0 &&
             s.v_head_stride >= 0 && s.qo_row_stride >= 0 && s.qo_head_stride >= 0 && s.ko_row_stride >= 0 && s.ko_head_stride >= 0 &&
             s.kc_batch_stride >= 0 && s.kc_row_stride >= 0 && s.kc_head_stride >= 0 && s.vc_batch_stride >= 0 &&
             s.vc_row_stride >= 0 && s.vc_head_stride >= 0, "%s strides must be non-negative", op);
    if (cached) FA_CHECK(s.page_block_size > 0, "%s: page_block_size must be positive (a contiguous cache: S_max)", op);
    FA_CHECK(((addr(s.q) | addr(s.k) | addr(s.v) | addr(s.q_out) | addr(s.k_out)) & 15) == 0 &&
             ((s.q_row_stride | s.q_head_stride | s.k_row_stride | s.k_head_stride | s.v_row_stride | s.v_head_stride |
               s.qo_row_stride | s.qo_head_stride | s.ko_row_stride | s.ko_head_stride) & 7) == 0,
             "%s: q / k / v / q_out / k_out base addresses and strides must be multiples of 16 bytes", op);
    const bool kv8 = cached && s.cache_dtype == FA_FP8_E4M3;
    if (cached) FA_TRY(check_cache_align(op, s, kv8));
    FA_CHECK(addr(s.positions) % 8 == 0 && addr(s.slot_mapping) % 8 == 0, "%s: positions and slot_mapping must be 8-byte aligned int64 arrays", op);
    FA_TRY(check_rope_align(op, s));
    FA_TRY(check_descales(op, s.k_descale, s.v_descale));
    if ((int64_t)(s.nheads_q + 2 * (int64_t)s.nheads_k) * s.head_dim > ((int64_t)1 << 24))
        return fail(FA_ERR_UNSUPPORTED, "%s: (nheads_q + 2 nheads_k) x head_dim is too large for one launch", op);
    if (!s.q) s.nheads_q = 0;
    const bool q_inplace = s.q && s.q_out == s.q, k_inplace = s.k_out == s.k;
    if (q_inplace)
        FA_CHECK(s.q_row_stride == s.qo_row_stride && s.q_head_stride == s.qo_head_stride,
                 "%s: q_out shares q's base address but not its strides (in place needs both equal)", op);
    if (k_inplace)
        FA_CHECK(s.k_row_stride == s.ko_row_stride && s.k_head_stride == s.ko_head_stride,
                 "%s: k_out shares k's base address but not its strides (in place needs both equal)", op);
    if (s.total_rows == 0 || s.head_dim == 0 || (s.nheads_q == 0 && s.nheads_k == 0)) { *empty = true; return FA_OK; }
    // an out-of-place output must not lie inside anything that is read or inside a cache: other workgroups still read and write
    // them.  One address range per tensor (an in-place output: empty, it is exempt)
    const int64_t T = s.total_rows, D = s.head_dim, Hq = s.nheads_q, Hk = s.nheads_k, half = s.rotary_dim / 2;
    const int csize = kv8 ? 1 : 2;
    const char* note = " without being in place (in place: the same base address and strides)";
    const View in[] = {
        view_flat("q", s.q, Hq ? span_bytes(1, 0, T, s.q_row_stride, Hq, s.q_head_stride, D, 2) : 0, note),
        view_flat("k", s.k, Hk ? span_bytes(1, 0, T, s.k_row_stride, Hk, s.k_head_stride, D, 2) : 0, note),
        view_flat("v", s.v, Hk ? span_bytes(1, 0, T, s.v_row_stride, Hk, s.v_head_stride, D, 2) : 0, note),
        view_flat("positions", s.positions, (uint64_t)T * 8, note),
        view_flat("slot_mapping", s.slot_mapping, (uint64_t)T * 8, note),
        view_flat("rotary_cos", s.rotary_cos, (uint64_t)s.seqlen_ro * half * 2, note),
        view_flat("rotary_sin", s.rotary_sin, (uint64_t)s.seqlen_ro * half * 2, note),
        view_flat("k_cache", s.k_cache, (Hk && s.num_blocks)
            ? span_bytes(s.num_blocks, s.kc_batch_stride, s.page_block_size, s.kc_row_stride, Hk, s.kc_head_stride, D, csize) : 0, note),
        view_flat("v_cache", s.v_cache, (Hk && s.num_blocks)
            ? span_bytes(s.num_blocks, s.vc_batch_stride, s.page_block_size, s.vc_row_stride, Hk, s.vc_head_stride, D, csize) : 0, note),
    };
    const View out[2] = {
        view_flat("q_out", s.q_out, (s.q && Hq && !q_inplace) ? span_bytes(1, 0, T, s.qo_row_stride, Hq, s.qo_head_stride, D, 2) : 0, note),
        view_flat("k_out", s.k_out, (Hk && !k_inplace) ? span_bytes(1, 0, T, s.ko_row_stride, Hk, s.ko_head_stride, D, 2) : 0, note),
    };
    for (const View& o : out) {                           // (q_out against everything, then k_out)
        FA_TRY(check_overlaps(op, &o, 1, in, (int)(sizeof(in) / sizeof(in[0])), false));
        FA_TRY(check_overlaps(op, &o, 1, extra, n_extra, false));
    }
    return FA_OK;
}

// fa_qk_norm_rope_store's argument rules: the norm's, then fa_rope_store's on the same block
static int qk_norm_rope_store_check(fa_qk_norm_rope_store_params& s, bool* empty) {
    const char* op = "qk_norm_rope_store";
    if (s.q_weight || s.k_weight) FA_TRY(check_weight_dtype(op, s.weight_dtype, s.dtype, "q / k dtype"));
    FA_CHECK(((addr(s.q_weight) | addr(s.k_weight)) & 15) == 0, "%s: q_weight / k_weight must be 16-byte aligned", op);
    FA_TRY(check_norm_scalars(op, s.eps, s.weight_offset));
    const uint64_t wbytes = (uint64_t)(s.head_dim > 0 ? s.head_dim : 0) * (s.weight_dtype == FA_FP32 ? 4 : 2);
    const View extra[2] = {view_flat("q_weight", s.q_weight, wbytes), view_flat("k_weight", s.k_weight, wbytes)};
    return rope_store_check(s, op, true, extra, 2, empty);
}

// fa_qk_norm_rope_bwd's argument rules (the forward's where the two ops share a field); normalises the block (no rotation: the
// pointers and rotary_dim cleared; no q: nheads_q = 0).  query: the workspace itself is not looked at
static int qk_norm_rope_bwd_check(fa_qk_norm_rope_bwd_params& s, bool query) {
    const char* op = "qk_norm_rope_bwd";
    FA_CHECK(s.k && s.dk_out, "%s: k and dk_out must not be NULL", op);
    FA_CHECK(!s.q || s.dq_out, "%s: q needs dq_out (a NULL q: no q heads)", op);
    FA_CHECK(!s.dq || s.q, "%s: dq needs q", op);
    FA_CHECK(!s.dq_weight || s.q_weight, "%s: dq_weight needs q_weight", op);
    FA_CHECK(!s.dk_weight || s.k_weight, "%s: dk_weight needs k_weight", op);
    FA_CHECK(s.reserved == 0 && s.reserved1[0] == 0 && s.reserved1[1] == 0, "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    bool no_rope;
    FA_TRY(check_rope_tables(op, s, true, &no_rope));
    FA_TRY(check_io_dtype(op, s.dtype, "q / k dtype"));
    if (s.q_weight || s.k_weight) FA_TRY(check_weight_dtype(op, s.weight_dtype, s.dtype, "q / k dtype"));
    FA_CHECK(s.total_rows >= 0 && s.nheads_q >= 0 && s.nheads_k >= 0 && s.head_dim >= 0 && s.seqlen_ro >= 0, "%s sizes must be non-negative", op);
    FA_CHECK(s.head_dim % 8 == 0 && s.head_dim <= 256, "%s head_dim must be a multiple of 8 and <= 256, got %d", op, s.head_dim);
    FA_TRY(check_rope_dims(op, s, no_rope));
    FA_CHECK(s.dqo_row_stride >= 0 && s.dqo_head_stride >= 0 && s.dko_row_stride >= 0 && s.dko_head_stride >= 0 && s.q_row_stride >= 0 &&
             s.q_head_stride >= 0 && s.k_row_stride >= 0 && s.k_head_stride >= 0 && s.dq_row_stride >= 0 && s.dq_head_stride >= 0 &&
             s.dk_row_stride >= 0 && s.dk_head_stride >= 0, "%s strides must be non-negative", op);
    FA_CHECK(((addr(s.dq_out) | addr(s.dk_out) | addr(s.q) | addr(s.k) | addr(s.dq) | addr(s.dk)) & 15) == 0 &&
             ((s.dqo_row_stride | s.dqo_head_stride | s.dko_row_stride | s.dko_head_stride | s.q_row_stride | s.q_head_stride |
               s.k_row_stride | s.k_head_stride | s.dq_row_stride | s.dq_head_stride | s.dk_row_stride | s.dk_head_stride) & 7) == 0,
             "%s: dq_out / dk_out / q / k / dq / dk base addresses and strides must be multiples of 16 bytes", op);
    FA_CHECK(addr(s.positions) % 8 == 0, "%s: positions must be an 8-byte aligned int64 array", op);
    FA_TRY(check_rope_align(op, s));
    FA_CHECK(((addr(s.q_weight) | addr(s.k_weight) | addr(s.dq_weight) | addr(s.dk_weight)) & 15) == 0,
             "%s: q_weight / k_weight / dq_weight / dk_weight must be 16-byte aligned", op);
    FA_TRY(check_norm_scalars(op, s.eps, s.weight_offset));
    if ((int64_t)(s.nheads_q + (int64_t)s.nheads_k) * s.head_dim > ((int64_t)1 << 24))
        return fail(FA_ERR_UNSUPPORTED, "%s: (nheads_q + nheads_k) x head_dim is too large for one launch", op);
    if (!s.q) { s.nheads_q = 0; s.dq_out = nullptr; }
    const bool q_inplace = s.dq && s.dq == s.dq_out, k_inplace = s.dk && s.dk == s.dk_out;
    if (q_inplace)
        FA_CHECK(s.dq_row_stride == s.dqo_row_stride && s.dq_head_stride == s.dqo_head_stride,
                 "%s: dq shares dq_out's base address but not its strides (in place needs both equal)", op);
    if (k_inplace)
        FA_CHECK(s.dk_row_stride == s.dko_row_stride && s.dk_head_stride == s.dko_head_stride,
                 "%s: dk shares dk_out's base address but not its strides (in place needs both equal)", op);
    const size_t need = fa::qk_norm_rope_bwd_workspace_bytes(s);
    if (query) return FA_OK;                              // (the query is about sizes: it does not look at where the tensors lie)
    if (need) {
        FA_CHECK(s.workspace && s.workspace_bytes >= need, "%s: the workspace holds %zu bytes, fa_qk_norm_rope_bwd_workspace_bytes() reports %zu",
                 op, s.workspace ? s.workspace_bytes : (size_t)0, need);
        FA_CHECK(addr(s.workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", op);
    }
    // an output must share no element with anything that is read (the exact in-place aliasing apart: that output is exempt, the
    // caller guarantees that its view shares no element with the others), with another output or with the workspace.  The q / k
    // tensors are [rows, heads, head_dim] views: the heads of one packed buffer are disjoint
    const int64_t T = s.total_rows, D = s.head_dim, Hq = s.nheads_q, Hk = s.nheads_k, half = s.rotary_dim / 2;
    const uint64_t wbytes = (uint64_t)D * (s.weight_dtype == FA_FP32 ? 4 : 2);
    const char* note = " without being in place (in place: the gradient's base address and strides)";
    auto heads = [D](const char* name, const void* p, int64_t rows, int64_t rs, int64_t h, int64_t hs, const char* nt = nullptr) {
        return view_rows(name, h > 0 && D > 0 ? p : nullptr, rows, rs, (h - 1) * hs + D, 2, nt);
    };
    const View in[] = {
        heads("dq_out", s.dq_out, T, s.dqo_row_stride, Hq, s.dqo_head_stride, note),
        heads("dk_out", s.dk_out, T, s.dko_row_stride, Hk, s.dko_head_stride, note),
        heads("q", s.q, T, s.q_row_stride, Hq, s.q_head_stride),
        heads("k", s.k, T, s.k_row_stride, Hk, s.k_head_stride),
        view_flat("positions", s.positions, (uint64_t)T * 8),
        view_flat("rotary_cos", s.rotary_cos, (uint64_t)s.seqlen_ro * half * 2),
        view_flat("rotary_sin", s.rotary_sin, (uint64_t)s.seqlen_ro * half * 2),
        view_flat("q_weight", s.q_weight, wbytes),
        view_flat("k_weight", s.k_weight, wbytes),
    };
    const View out[] = {
        heads("dq", q_inplace ? nullptr : s.dq, T, s.dq_row_stride, Hq, s.dq_head_stride, note),
        heads("dk", k_inplace ? nullptr : s.dk, T, s.dk_row_stride, Hk, s.dk_head_stride, note),
        view_flat("dq_weight", s.dq_weight, wbytes),
        view_flat("dk_weight", s.dk_weight, wbytes),
        view_flat("workspace", need ? s.workspace : nullptr, need),
    };
    return check_overlaps(op, out, (int)(sizeof(out) / sizeof(out[0])), in, (int)(sizeof(in) / sizeof(in[0])), true);
}

static bool an_is_io_or_fp32(int t, int dtype) { return t == dtype || t == FA_FP32; }
static bool an_stride_ok(int64_t rs, int64_t rows, int n) { return rs >= 0 && rs % 8 == 0 && (rows <= 1 || rs >= n); }

// what fa_add_norm and fa_add_norm_bwd share: dtype, n, rows, the weight, eps, weight_offset
static int add_norm_common_check(const char* op, int dtype, int weight_dtype, int64_t rows, int n, const void* weight, float eps,
                                 float weight_offset) {
    FA_TRY(check_io_dtype(op, dtype, "dtype"));
    FA_TRY(check_weight_dtype(op, weight_dtype, dtype, "io dtype"));
    FA_CHECK(weight, "%s: weight must not be NULL", op);
    FA_CHECK(rows >= 0, "%s: rows must be non-negative", op);
    FA_CHECK(n >= 8 && n <= 16384 && n % 8 == 0, "%s: n must be a multiple of 8 in [8, 16384], got %d", op, n);
    return check_norm_scalars(op, eps, weight_offset);
}

// fa_add_norm's argument rules.  quant_out (fa_add_norm_quant): the n_quant views - codes, scales - that take the place of `out`,
// which must be NULL then
static int add_norm_check(const fa_add_norm_params& s, const char* op = "add_norm", const View* quant_out = nullptr, int n_quant = 0) {
    if (quant_out) {
        FA_CHECK(s.x, "%s: x must not be NULL", op);
        FA_CHECK(!s.out && s.out_row_stride == 0, "%s: norm.out must be NULL and norm.out_row_stride 0 (codes take its place)", op);
    } else {
        FA_CHECK(s.x && s.out, "%s: x and out must not be NULL", op);
    }
    FA_CHECK(!s.residual || s.residual_out, "%s: a residual needs residual_out", op);
    FA_CHECK(s.reserved[0] == 0 && s.reserved[1] == 0, "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(add_norm_common_check(op, s.dtype, s.weight_dtype, s.rows, s.n, s.weight, s.eps, s.weight_offset));
    if (s.residual) FA_CHECK(an_is_io_or_fp32(s.residual_dtype, s.dtype), "%s: residual_dtype must be the io dtype or fp32", op);
    if (s.residual_out) {
        FA_CHECK(an_is_io_or_fp32(s.residual_out_dtype, s.dtype), "%s: residual_out_dtype must be the io dtype or fp32", op);
        FA_CHECK(!s.residual || s.residual_dtype != FA_FP32 || s.residual_out_dtype == FA_FP32,
                 "%s: an fp32 residual needs an fp32 residual_out", op);
    }
    FA_CHECK(an_stride_ok(s.x_row_stride, s.rows, s.n) && (quant_out || an_stride_ok(s.out_row_stride, s.rows, s.n)) &&
             (!s.residual || an_stride_ok(s.residual_row_stride, s.rows, s.n)) &&
             (!s.residual_out || an_stride_ok(s.residual_out_row_stride, s.rows, s.n)),
             "%s: row strides must be non-negative multiples of 8 elements and (rows > 1) at least n", op);
    FA_CHECK(((addr(s.x) | addr(s.out) | addr(s.residual) | addr(s.residual_out) | addr(s.weight) | addr(s.bias)) & 15) == 0,
             "%s: x / residual / out / residual_out / weight / bias must be 16-byte aligned", op);
    if (s.rows > 0x7fffffffLL) return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 rows in one launch", op);
    const bool x_inplace = s.out && s.out == s.x, r_inplace = s.residual_out && s.residual_out == s.residual;
    if (x_inplace) FA_CHECK(s.out_row_stride == s.x_row_stride, "%s: out shares x's base address but not its row stride (in place needs both equal)", op);
    if (r_inplace)
        FA_CHECK(s.residual_out_row_stride == s.residual_row_stride && s.residual_out_dtype == s.residual_dtype,
                 "%s: residual_out shares residual's base address but not its row stride and dtype (in place needs all equal)", op);
    // [rows, n] views: column ranges of one wider buffer are disjoint
    const int rsz = s.residual_dtype == FA_FP32 ? 4 : 2, rosz = s.residual_out_dtype == FA_FP32 ? 4 : 2;
    const uint64_t wbytes = (uint64_t)s.n * (s.weight_dtype == FA_FP32 ? 4 : 2);
    const char* note = " (in place needs the same base address, row stride and dtype)";
    const View in[] = {
        view_rows("x", s.x, s.rows, s.x_row_stride, s.n, 2, note),
        view_rows("residual", s.residual, s.rows, s.residual_row_stride, s.n, rsz, note),
        view_flat("weight", s.weight, wbytes, note),
        view_flat("bias", s.bias, wbytes, note),
    };
    View out[4] = {
        view_rows("out", s.out, s.rows, s.out_row_stride, s.n, 2, note),
        view_rows("residual_out", s.residual_out, s.rows, s.residual_out_row_stride, s.n, rosz, note),
    };
    for (int i = 0; i < n_quant && i < 2; ++i) out[2 + i] = quant_out[i];
    int exempt[2][2], n_ex = 0;
    if (x_inplace) { exempt[n_ex][0] = 0; exempt[n_ex++][1] = 0; }
    if (r_inplace) { exempt[n_ex][0] = 1; exempt[n_ex++][1] = 1; }
    return check_overlaps(op, out, 2 + (n_quant < 2 ? n_quant : 2), in, 4, true, exempt, n_ex);
}

// fa_add_norm_bwd's argument rules.  query: the workspace itself and where the tensors lie are not looked at
static int add_norm_bwd_check(const fa_add_norm_bwd_params& s, bool query) {
    const char* op = "add_norm_bwd";
    FA_CHECK(s.dy && s.z, "%s: dy and z must not be NULL", op);
    FA_CHECK(s.reserved[0] == 0 && s.reserved[1] == 0, "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(add_norm_common_check(op, s.dtype, s.weight_dtype, s.rows, s.n, s.weight, s.eps, s.weight_offset));
    FA_CHECK(an_is_io_or_fp32(s.z_dtype, s.dtype), "%s: z_dtype must be the io dtype or fp32", op);
    if (s.dres) FA_CHECK(an_is_io_or_fp32(s.dres_dtype, s.dtype), "%s: dres_dtype must be the io dtype or fp32", op);
    FA_CHECK(an_stride_ok(s.dy_row_stride, s.rows, s.n) && an_stride_ok(s.z_row_stride, s.rows, s.n) &&
             (!s.dres_out || an_stride_ok(s.dres_out_row_stride, s.rows, s.n)) && (!s.dx || an_stride_ok(s.dx_row_stride, s.rows, s.n)) &&
             (!s.dres || an_stride_ok(s.dres_row_stride, s.rows, s.n)),
             "%s: row strides must be non-negative multiples of 8 elements and (rows > 1) at least n", op);
    FA_CHECK(((addr(s.dy) | addr(s.z) | addr(s.dres_out) | addr(s.dx) | addr(s.dres) | addr(s.weight) | addr(s.dweight) | addr(s.dbias)) & 15) == 0,
             "%s: dy / z / dres_out / dx / dres / weight / dweight / dbias must be 16-byte aligned", op);
    if (s.rows > 0x7fffffffLL) return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 rows in one launch", op);
    const bool inplace = s.dx && s.dx == s.dy;
    if (inplace) FA_CHECK(s.dx_row_stride == s.dy_row_stride, "%s: dx shares dy's base address but not its row stride (in place needs both equal)", op);
    if (query) return FA_OK;
    const size_t need = fa::add_norm_bwd_workspace_bytes(s);
    if (need) {
        FA_CHECK(s.workspace && s.workspace_bytes >= need, "%s: the workspace holds %zu bytes, fa_add_norm_bwd_workspace_bytes() reports %zu",
                 op, s.workspace ? s.workspace_bytes : (size_t)0, need);
        FA_CHECK(addr(s.workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", op);
    }
    const int zsz = s.z_dtype == FA_FP32 ? 4 : 2, dsz = s.dres_dtype == FA_FP32 ? 4 : 2;
    const uint64_t wbytes = (uint64_t)s.n * (s.weight_dtype == FA_FP32 ? 4 : 2);
    const char* note = " (in place needs the same base address, row stride and dtype)";
    const View in[] = {
        view_rows("dy", s.dy, s.rows, s.dy_row_stride, s.n, 2, note),
        view_rows("z", s.z, s.rows, s.z_row_stride, s.n, zsz, note),
        view_rows("dres_out", s.dres_out, s.rows, s.dres_out_row_stride, s.n, zsz, note),
        view_flat("weight", s.weight, wbytes, note),
    };
    const View out[] = {
        view_rows("dx", s.dx, s.rows, s.dx_row_stride, s.n, 2, note),
        view_rows("dres", s.dres, s.rows, s.dres_row_stride, s.n, dsz, note),
        view_flat("dweight", s.dweight, wbytes, note),
        view_flat("dbias", s.dbias, wbytes, note),
        view_flat("workspace", need ? s.workspace : nullptr, need, note),
    };
    const int exempt[1][2] = {{0, 0}};
    return check_overlaps(op, out, 5, in, 4, true, exempt, inplace ? 1 : 0);
}

// what fa_cross_entropy and fa_cross_entropy_bwd share: dtype, vocab, rows, the scalars.  Returns the logits' element size
static int cross_entropy_common_check(const char* op, int dtype, int vocab, int64_t rows, float label_smoothing, float logit_scale,
                                      float lse_square_scale, int* esize) {
    FA_CHECK(dtype == FA_FP16 || dtype == FA_BF16 || dtype == FA_FP32, "%s: dtype must be fp16, bf16 or fp32", op);
    *esize = dtype == FA_FP32 ? 4 : 2;
    FA_CHECK(vocab >= 1, "%s: vocab must be at least 1, got %d", op, vocab);
    FA_CHECK(rows >= 0, "%s: rows must be non-negative", op);
    FA_CHECK(label_smoothing >= 0.f && label_smoothing < 1.f, "%s: label_smoothing must be in [0, 1)", op);
    FA_CHECK(logit_scale >= -3.402823466e38f && logit_scale <= 3.402823466e38f, "%s: logit_scale must be finite", op);
    FA_CHECK(lse_square_scale >= 0.f && lse_square_scale <= 3.402823466e38f, "%s: lse_square_scale must be finite and >= 0", op);
    return FA_OK;
}
static bool ce_stride_ok(int64_t rs, int64_t rows, int vocab) { return rs >= 0 && (rows <= 1 || rs >= vocab); }

// fa_cross_entropy's argument rules.  query: the workspace itself and where the tensors lie are not looked at
static int cross_entropy_check(const fa_cross_entropy_params& s, bool query) {
    const char* op = "cross_entropy";
    FA_CHECK(s.logits && s.labels && s.losses && s.z_losses && s.lse, "%s: logits, labels, losses, z_losses and lse must not be NULL", op);
    FA_CHECK(s.reserved0 == 0 && s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    int esize;
    FA_TRY(cross_entropy_common_check(op, s.dtype, s.vocab, s.rows, s.label_smoothing, s.logit_scale, s.lse_square_scale, &esize));
    FA_CHECK(ce_stride_ok(s.logits_row_stride, s.rows, s.vocab), "%s: the row stride must be non-negative and (rows > 1) at least vocab", op);
    FA_CHECK(addr(s.logits) % esize == 0 && addr(s.labels) % 8 == 0 && ((addr(s.losses) | addr(s.z_losses) | addr(s.lse)) & 3) == 0,
             "%s: logits must be aligned to their element, labels to 8 bytes, losses / z_losses / lse to 4 bytes", op);
    const int64_t nc = fa::ce_nchunks(s.vocab, s.dtype);
    if (s.rows > 0x7fffffffLL / nc) return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups (rows x chunks) in one launch", op);
    if (query) return FA_OK;
    const size_t need = fa::cross_entropy_workspace_bytes(s.rows, s.vocab, s.dtype);
    if (need) {
        FA_CHECK(s.workspace && s.workspace_bytes >= need, "%s: the workspace holds %zu bytes, fa_cross_entropy_workspace_bytes() reports %zu",
                 op, s.workspace ? s.workspace_bytes : (size_t)0, need);
        FA_CHECK(addr(s.workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", op);
    }
    const uint64_t vbytes = s.rows > 0 ? (uint64_t)s.rows * 4 : 0;
    const View in[] = {
        view_rows("logits", s.logits, s.rows, s.logits_row_stride, s.vocab, esize),
        view_flat("labels", s.labels, 2 * vbytes),
    };
    const View out[] = {
        view_flat("losses", s.losses, vbytes),
        view_flat("z_losses", s.z_losses, vbytes),
        view_flat("lse", s.lse, vbytes),
        view_flat("workspace", need ? s.workspace : nullptr, need),
    };
    return check_overlaps(op, out, 4, in, 2, true);
}

// fa_cross_entropy_bwd's argument rules
static int cross_entropy_bwd_check(const fa_cross_entropy_bwd_params& s) {
    const char* op = "cross_entropy_bwd";
    FA_CHECK(s.dlosses && s.logits && s.labels && s.lse && s.dlogits, "%s: dlosses, logits, labels, lse and dlogits must not be NULL", op);
    FA_CHECK(s.reserved0 == 0 && s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    int esize;
    FA_TRY(cross_entropy_common_check(op, s.dtype, s.vocab, s.rows, s.label_smoothing, s.logit_scale, s.lse_square_scale, &esize));
    FA_CHECK(ce_stride_ok(s.logits_row_stride, s.rows, s.vocab) && ce_stride_ok(s.dlogits_row_stride, s.rows, s.vocab),
             "%s: row strides must be non-negative and (rows > 1) at least vocab", op);
    FA_CHECK(s.dlosses_stride >= 0, "%s: dlosses_stride must be non-negative", op);
    FA_CHECK(addr(s.logits) % esize == 0 && addr(s.dlogits) % esize == 0 && addr(s.labels) % 8 == 0 && ((addr(s.dlosses) | addr(s.lse)) & 3) == 0,
             "%s: logits / dlogits must be aligned to their element, labels to 8 bytes, dlosses / lse to 4 bytes", op);
    if (s.rows > 0x7fffffffLL / fa::ce_bwd_nchunks(s.vocab))
        return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups (rows x chunks) in one launch", op);
    const bool inplace = s.dlogits == s.logits;
    if (inplace) FA_CHECK(s.dlogits_row_stride == s.logits_row_stride,
                          "%s: dlogits shares logits' base address but not its row stride (in place needs both equal)", op);
    const uint64_t vbytes = s.rows > 0 ? (uint64_t)s.rows * 4 : 0;
    const char* note = " (in place needs the same base address and row stride)";
    const View in[] = {
        view_rows("logits", s.logits, s.rows, s.logits_row_stride, s.vocab, esize, note),
        view_rows("dlosses", s.dlosses, s.rows, s.dlosses_stride, 1, 4),
        view_flat("labels", s.labels, 2 * vbytes),
        view_flat("lse", s.lse, vbytes),
    };
    const View out = view_rows("dlogits", s.dlogits, s.rows, s.dlogits_row_stride, s.vocab, esize, note);
    const int exempt[1][2] = {{0, 0}};
    return check_overlaps(op, &out, 1, in, 4, false, exempt, inplace ? 1 : 0);
}

// fa_sample's argument rules.  query: the workspace itself and where the tensors lie are not looked at
static int sample_check(const fa_sample_params& s, bool query) {
    const char* op = "sample";
    FA_CHECK(s.logits, "%s: logits must not be NULL", op);
    FA_CHECK(s.ids || s.filtered, "%s: at least one of ids and filtered must be given", op);
    FA_CHECK(s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_CHECK(s.dtype == FA_FP16 || s.dtype == FA_BF16 || s.dtype == FA_FP32, "%s: dtype must be fp16, bf16 or fp32", op);
    const int esize = s.dtype == FA_FP32 ? 4 : 2;
    FA_CHECK(s.vocab >= 1, "%s: vocab must be at least 1, got %d", op, s.vocab);
    FA_CHECK(s.rows >= 0, "%s: rows must be non-negative", op);
    // (a row that is greedy whatever its logits - the host temperature is not above 0 - never reads u)
    FA_CHECK(!s.ids || s.u || (!s.temperature && !(s.temperature_value > 0.f)),
             "%s: ids needs u (one uniform number per row) unless the temperature is the host scalar 0", op);
    FA_CHECK(ce_stride_ok(s.logits_row_stride, s.rows, s.vocab) && (!s.filtered || ce_stride_ok(s.filtered_row_stride, s.rows, s.vocab)),
             "%s: row strides must be non-negative and (rows > 1) at least vocab", op);
    FA_CHECK(addr(s.logits) % esize == 0 && addr(s.filtered) % esize == 0 &&
             ((addr(s.u) | addr(s.temperature) | addr(s.top_k) | addr(s.top_p) | addr(s.min_p) | addr(s.ids) | addr(s.n_kept) | addr(s.lse)) & 3) == 0,
             "%s: logits / filtered must be aligned to their element, every [rows] array to 4 bytes", op);
    if (s.vocab > (1 << 20)) return fail(FA_ERR_UNSUPPORTED, "%s: vocab %d is above 2^20 (the integer masses of a row must fit 64 bits)", op, s.vocab);
    if (s.rows > 0x7fffffffLL / fa::sample_chunks_per_row(s.vocab))
        return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups (rows x chunks) in one launch", op);
    if (query) return FA_OK;
    const size_t need = fa::sample_workspace_bytes(s.rows, s.vocab, s.dtype);
    if (need)
        FA_CHECK(s.workspace && s.workspace_bytes >= need, "%s: the workspace holds %zu bytes, fa_sample_workspace_bytes() reports %zu",
                 op, s.workspace ? s.workspace_bytes : (size_t)0, need);
    FA_CHECK(addr(s.workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", op);
    const uint64_t vbytes = s.rows > 0 ? (uint64_t)s.rows * 4 : 0;
    const View in[] = {
        view_rows("logits", s.logits, s.rows, s.logits_row_stride, s.vocab, esize),
        view_flat("u", s.u, vbytes),
        view_flat("temperature", s.temperature, vbytes),
        view_flat("top_k", s.top_k, vbytes),
        view_flat("top_p", s.top_p, vbytes),
        view_flat("min_p", s.min_p, vbytes),
    };
    const View out[] = {
        view_rows("filtered", s.filtered, s.rows, s.filtered_row_stride, s.vocab, esize),
        view_flat("ids", s.ids, vbytes),
        view_flat("n_kept", s.n_kept, vbytes),
        view_flat("lse", s.lse, vbytes),
        view_flat("workspace", need ? s.workspace : nullptr, need),
    };
    return check_overlaps(op, out, 5, in, 6, true);
}

// fa_spec_accept's argument rules.  query: the workspace itself and where the tensors lie are not looked at
static int spec_accept_check(const fa_spec_accept_params& s, bool query) {
    const char* op = "spec_accept";
    FA_CHECK(s.target_logits && s.draft_probs && s.draft_ids && s.accept && s.recovered,
             "%s: target_logits, draft_probs, draft_ids, accept and recovered must not be NULL", op);
    FA_CHECK(s.reserved0 == 0 && s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_CHECK(s.dtype == FA_FP16 || s.dtype == FA_BF16 || s.dtype == FA_FP32, "%s: dtype must be fp16, bf16 or fp32", op);
    FA_CHECK(s.probs_dtype == FA_FP16 || s.probs_dtype == FA_BF16 || s.probs_dtype == FA_FP32, "%s: probs_dtype must be fp16, bf16 or fp32", op);
    const int esize = s.dtype == FA_FP32 ? 4 : 2, qsize = s.probs_dtype == FA_FP32 ? 4 : 2;
    FA_CHECK(s.nodes >= 1 && s.nodes <= 64, "%s: nodes must be in 1 .. 64, got %d", op, s.nodes);
    FA_CHECK(s.vocab >= 1, "%s: vocab must be at least 1, got %d", op, s.vocab);
    FA_CHECK(s.batch >= 0, "%s: batch must be non-negative", op);
    // (a node that is greedy whatever its logits - the host temperature is not above 0 - never reads the uniform numbers)
    FA_CHECK((s.u_accept && s.u_recover) || (!s.temperature && !(s.temperature_value > 0.f)),
             "%s: u_accept and u_recover are needed unless the temperature is the host scalar 0", op);
    if (s.batch > 0x7fffffffLL / s.nodes) return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 nodes in one launch", op);
    const int64_t rows = s.batch * s.nodes;
    FA_CHECK(ce_stride_ok(s.logits_row_stride, rows, s.vocab) && ce_stride_ok(s.probs_row_stride, rows, s.vocab),
             "%s: row strides must be non-negative and (batch x nodes > 1) at least vocab", op);
    FA_CHECK(s.parents_batch_stride >= 0, "%s: parents_batch_stride must be non-negative", op);
    FA_CHECK(addr(s.target_logits) % esize == 0 && addr(s.draft_probs) % qsize == 0 &&
             ((addr(s.draft_ids) | addr(s.parents) | addr(s.u_accept) | addr(s.u_recover) | addr(s.temperature) | addr(s.accept) | addr(s.recovered)) & 3) == 0,
             "%s: target_logits / draft_probs must be aligned to their element, every int32 / fp32 array to 4 bytes", op);
    if (s.vocab > (1 << 20)) return fail(FA_ERR_UNSUPPORTED, "%s: vocab %d is above 2^20 (the integer masses of a row must fit 64 bits)", op, s.vocab);
    if (rows > 0x7fffffffLL / fa::spec_accept_chunks(s.vocab))
        return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups (nodes x chunks) in one launch", op);
    if (query) return FA_OK;
    const size_t need = fa::spec_accept_workspace_bytes(rows, s.vocab);
    if (need)
        FA_CHECK(s.workspace && s.workspace_bytes >= need, "%s: the workspace holds %zu bytes, fa_spec_accept_workspace_bytes() reports %zu",
                 op, s.workspace ? s.workspace_bytes : (size_t)0, need);
    FA_CHECK(addr(s.workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", op);
    const uint64_t vbytes = (uint64_t)rows * 4;
    const uint64_t pbytes = rows > 0 ? (uint64_t)((s.batch - 1) * s.parents_batch_stride + s.nodes) * 4 : 0;
    const View in[] = {
        view_rows("target_logits", s.target_logits, rows, s.logits_row_stride, s.vocab, esize),
        view_rows("draft_probs", s.draft_probs, rows, s.probs_row_stride, s.vocab, qsize),
        view_flat("draft_ids", s.draft_ids, vbytes),
        view_flat("parents", s.parents, pbytes),
        view_flat("u_accept", s.u_accept, vbytes),
        view_flat("u_recover", s.u_recover, vbytes),
        view_flat("temperature", s.temperature, s.batch > 0 ? (uint64_t)s.batch * 4 : 0),
    };
    const View out[] = {
        view_flat("accept", s.accept, vbytes),
        view_flat("recovered", s.recovered, vbytes),
        view_flat("workspace", need ? s.workspace : nullptr, need),
    };
    return check_overlaps(op, out, 3, in, 7, true);
}

// fa_spec_walk's argument rules
static int spec_walk_check(const fa_spec_walk_params& s) {
    const char* op = "spec_walk";
    FA_CHECK(s.draft_ids && s.target_ids && s.out_tokens && s.num_out && s.path_nodes,
             "%s: draft_ids, target_ids, out_tokens, num_out and path_nodes must not be NULL", op);
    FA_CHECK(!s.accept == !s.recovered, "%s: accept and recovered go together (both, or neither: deterministic drafts)", op);
    FA_CHECK(s.reserved0 == 0 && s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_CHECK(s.nodes >= 1 && s.nodes <= 64, "%s: nodes must be in 1 .. 64, got %d", op, s.nodes);
    FA_CHECK(s.batch >= 0, "%s: batch must be non-negative", op);
    FA_CHECK(s.parents_batch_stride >= 0 && s.target_ids_batch_stride >= 0 && s.target_ids_node_stride >= 0,
             "%s: strides must be non-negative", op);
    FA_CHECK(((addr(s.parents) | addr(s.draft_ids) | addr(s.target_ids) | addr(s.accept) | addr(s.recovered) | addr(s.out_tokens) |
               addr(s.num_out) | addr(s.path_nodes)) & 3) == 0, "%s: every array must be 4-byte aligned", op);
    if (s.batch > 0x7fffffffLL / s.nodes) return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 nodes in one launch", op);
    const bool any = s.batch > 0;
    const uint64_t vbytes = any ? (uint64_t)s.batch * s.nodes * 4 : 0;
    const uint64_t pbytes = any ? (uint64_t)((s.batch - 1) * s.parents_batch_stride + s.nodes) * 4 : 0;
    const uint64_t tbytes = any ? (uint64_t)((s.batch - 1) * s.target_ids_batch_stride + (s.nodes - 1) * s.target_ids_node_stride + 1) * 4 : 0;
    const View in[] = {
        view_flat("parents", s.parents, pbytes),
        view_flat("draft_ids", s.draft_ids, vbytes),
        view_flat("target_ids", s.target_ids, tbytes),
        view_flat("accept", s.accept, vbytes),
        view_flat("recovered", s.recovered, vbytes),
    };
    const View out[] = {
        view_flat("out_tokens", s.out_tokens, vbytes),
        view_flat("num_out", s.num_out, any ? (uint64_t)s.batch * 4 : 0),
        view_flat("path_nodes", s.path_nodes, vbytes),
    };
    return check_overlaps(op, out, 3, in, 5, true);
}

// what fa_act_mul and fa_act_mul_bwd share: dtype, activation, n, rows, and that rows x runs fits a grid index
static int act_mul_common_check(const char* op, int dtype, int activation, int n, int64_t rows) {
    FA_TRY(check_io_dtype(op, dtype, "dtype"));
    FA_CHECK(activation >= FA_ACT_SILU && activation <= FA_ACT_RELU2, "%s: unknown activation %d", op, activation);
    FA_CHECK(n >= 1, "%s: n must be at least 1, got %d", op, n);
    FA_CHECK(rows >= 0, "%s: rows must be non-negative", op);
    if (rows > 0x7fffffffLL / fa::act_plan(0, n).nchunks)
        return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 items (rows x runs per row) in one launch", op);
    return FA_OK;
}
static bool act_stride_ok(const void* p, int64_t rs, int64_t rows, int n) { return !p || (rs >= 0 && (rows <= 1 || rs >= n)); }

// the exact in-place pair (out, in): the same base address needs the same row stride
static int act_inplace(const char* op, const char* out_name, const void* out, int64_t out_rs, const char* in_name, const void* in,
                       int64_t in_rs, bool* inplace) {
    *inplace = out && out == in;
    if (*inplace) FA_CHECK(out_rs == in_rs, "%s: %s shares %s's base address but not its row stride (in place needs both equal)", op,
                           out_name, in_name);
    return FA_OK;
}

static const char* const kActNote = " (in place needs the same base address and row stride)";

// fa_act_mul's argument rules
static int act_mul_check(const fa_act_mul_params& s) {
    const char* op = "act_mul";
    FA_CHECK(s.gate && s.out, "%s: gate and out must not be NULL", op);
    FA_CHECK(s.reserved0 == 0 && s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(act_mul_common_check(op, s.dtype, s.activation, s.n, s.rows));
    FA_CHECK(act_stride_ok(s.gate, s.gate_row_stride, s.rows, s.n) && act_stride_ok(s.up, s.up_row_stride, s.rows, s.n) &&
             act_stride_ok(s.out, s.out_row_stride, s.rows, s.n), "%s: row strides must be non-negative and (rows > 1) at least n", op);
    FA_CHECK(((addr(s.gate) | addr(s.up) | addr(s.out)) & 1) == 0, "%s: gate / up / out must be aligned to their element", op);
    bool on_gate, on_up;
    FA_TRY(act_inplace(op, "out", s.out, s.out_row_stride, "gate", s.gate, s.gate_row_stride, &on_gate));
    FA_TRY(act_inplace(op, "out", s.out, s.out_row_stride, "up", s.up, s.up_row_stride, &on_up));
    const View in[] = {
        view_rows("gate", s.gate, s.rows, s.gate_row_stride, s.n, 2, kActNote),
        view_rows("up", s.up, s.rows, s.up_row_stride, s.n, 2, kActNote),
    };
    const View out = view_rows("out", s.out, s.rows, s.out_row_stride, s.n, 2, kActNote);
    int exempt[2][2], n_ex = 0;                             // {output, input}
    if (on_gate) { exempt[n_ex][0] = 0; exempt[n_ex++][1] = 0; }
    if (on_up) { exempt[n_ex][0] = 0; exempt[n_ex++][1] = 1; }
    return check_overlaps(op, &out, 1, in, 2, false, exempt, n_ex);
}

// fa_act_mul_bwd's argument rules
static int act_mul_bwd_check(const fa_act_mul_bwd_params& s) {
    const char* op = "act_mul_bwd";
    FA_CHECK(s.dout && s.gate && s.dgate, "%s: dout, gate and dgate must not be NULL", op);
    FA_CHECK((s.up == nullptr) == (s.dup == nullptr), "%s: up and dup go together (both, or both NULL: the ungated form)", op);
    FA_CHECK(s.reserved0 == 0 && s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(act_mul_common_check(op, s.dtype, s.activation, s.n, s.rows));
    FA_CHECK(act_stride_ok(s.dout, s.dout_row_stride, s.rows, s.n) && act_stride_ok(s.gate, s.gate_row_stride, s.rows, s.n) &&
             act_stride_ok(s.up, s.up_row_stride, s.rows, s.n) && act_stride_ok(s.dgate, s.dgate_row_stride, s.rows, s.n) &&
             act_stride_ok(s.dup, s.dup_row_stride, s.rows, s.n), "%s: row strides must be non-negative and (rows > 1) at least n", op);
    FA_CHECK(((addr(s.dout) | addr(s.gate) | addr(s.up) | addr(s.dgate) | addr(s.dup)) & 1) == 0,
             "%s: dout / gate / up / dgate / dup must be aligned to their element", op);
    bool on_gate, on_up;
    FA_TRY(act_inplace(op, "dgate", s.dgate, s.dgate_row_stride, "gate", s.gate, s.gate_row_stride, &on_gate));
    FA_TRY(act_inplace(op, "dup", s.dup, s.dup_row_stride, "up", s.up, s.up_row_stride, &on_up));
    const View in[] = {
        view_rows("gate", s.gate, s.rows, s.gate_row_stride, s.n, 2, kActNote),
        view_rows("up", s.up, s.rows, s.up_row_stride, s.n, 2, kActNote),
        view_rows("dout", s.dout, s.rows, s.dout_row_stride, s.n, 2),
    };
    const View out[] = {
        view_rows("dgate", s.dgate, s.rows, s.dgate_row_stride, s.n, 2, kActNote),
        view_rows("dup", s.dup, s.rows, s.dup_row_stride, s.n, 2, kActNote),
    };
    int exempt[2][2], n_ex = 0;                             // {output, input}
    if (on_gate) { exempt[n_ex][0] = 0; exempt[n_ex++][1] = 0; }
    if (on_up) { exempt[n_ex][0] = 1; exempt[n_ex++][1] = 1; }
    return check_overlaps(op, out, 2, in, 3, true, exempt, n_ex);
}

// ---- fa_quant_fp8, fa_add_norm_quant, fa_act_mul_quant
// the quantisation fields the three blocks share: mode, scale, scale_ub, the scales pointer and n against the mode
static int quant_rule_check(const char* op, int mode, int has_scale_ub, float scale, float scale_ub, const void* codes, const void* scales,
                            int n) {
    FA_CHECK(mode == FA_QUANT_ROW || mode == FA_QUANT_GROUP || mode == FA_QUANT_STATIC, "%s: unknown mode %d", op, mode);
    FA_CHECK(codes, "%s: codes must not be NULL", op);
    FA_CHECK(has_scale_ub == 0 || has_scale_ub == 1, "%s: has_scale_ub must be 0 or 1", op);
    if (mode == FA_QUANT_STATIC) {
        FA_CHECK(scale > 0.f && scale <= 3.402823466e38f, "%s: the static mode needs a scale that is finite and > 0", op);
        FA_CHECK(!has_scale_ub && scale_ub == 0.f, "%s: scale_ub goes with the dynamic modes (the static mode takes none)", op);
        FA_CHECK(!scales, "%s: scales must be NULL in the static mode (none is written)", op);
    } else {
        FA_CHECK(scale == 0.f, "%s: scale is given in the static mode only (the dynamic modes compute it; pass 0)", op);
        if (has_scale_ub) FA_CHECK(scale_ub > 0.f && scale_ub <= 3.402823466e38f, "%s: scale_ub must be finite and > 0", op);
        else              FA_CHECK(scale_ub == 0.f, "%s: scale_ub must be 0 where has_scale_ub is 0", op);
        FA_CHECK(scales, "%s: scales must not be NULL in the row and group modes", op);
        FA_CHECK((addr(scales) & 3) == 0, "%s: scales must be 4-byte aligned", op);
    }
    if (mode == FA_QUANT_GROUP) FA_CHECK(n % 128 == 0, "%s: the group mode needs n to be a multiple of 128, got %d", op, n);
    return FA_OK;
}
static int quant_n_check(const char* op, int n) {
    FA_CHECK(n >= 8 && n <= 65536 && n % 8 == 0, "%s: n must be a multiple of 8 in [8, 65536], got %d", op, n);
    return FA_OK;
}
// the scales a mode writes, as the overlap rules see them
static View quant_scales_view(const void* scales, int mode, int64_t rows, int n) {
    const uint64_t count = mode == FA_QUANT_GROUP ? (uint64_t)rows * (uint64_t)(n / 128) : (uint64_t)rows;
    return view_flat("scales", mode == FA_QUANT_STATIC ? nullptr : scales, count * 4);
}

// fa_quant_fp8's argument rules
static int quant_fp8_check(const fa_quant_fp8_params& s) {
    const char* op = "quant_fp8";
    FA_CHECK(s.x, "%s: x must not be NULL", op);
    FA_CHECK(s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(check_io_dtype(op, s.dtype, "dtype"));
    FA_TRY(quant_n_check(op, s.n));
    FA_TRY(quant_rule_check(op, s.mode, s.has_scale_ub, s.scale, s.scale_ub, s.codes, s.scales, s.n));
    FA_CHECK(s.rows >= 0, "%s: rows must be non-negative", op);
    FA_CHECK(act_stride_ok(s.x, s.x_row_stride, s.rows, s.n) && act_stride_ok(s.codes, s.codes_row_stride, s.rows, s.n),
             "%s: row strides must be non-negative and (rows > 1) at least n", op);
    FA_CHECK((addr(s.x) & 1) == 0, "%s: x must be aligned to its element", op);
    if (s.rows > 0x7fffffffLL) return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 rows in one launch", op);
    const View in = view_rows("x", s.x, s.rows, s.x_row_stride, s.n, 2);
    const View out[] = {
        view_rows("codes", s.codes, s.rows, s.codes_row_stride, s.n, 1),
        quant_scales_view(s.scales, s.mode, s.rows, s.n),
    };
    return check_overlaps(op, out, 2, &in, 1, true);
}

// fa_add_norm_quant's argument rules: fa_add_norm's on `norm`, codes and scales in the place of out
static int add_norm_quant_check(const fa_add_norm_quant_params& s) {
    const char* op = "add_norm_quant";
    FA_CHECK(s.norm.struct_size >= sizeof(fa_add_norm_params), "%s: norm.struct_size %zu is smaller than this library's %zu", op,
             s.norm.struct_size, sizeof(fa_add_norm_params));
    FA_CHECK(s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(add_norm_common_check(op, s.norm.dtype, s.norm.weight_dtype, s.norm.rows, s.norm.n, s.norm.weight, s.norm.eps,
                                 s.norm.weight_offset));                       // (n and rows first: the rules below read them)
    FA_TRY(quant_rule_check(op, s.mode, s.has_scale_ub, s.scale, s.scale_ub, s.codes, s.scales, s.norm.n));
    FA_CHECK((addr(s.codes) & 7) == 0 && s.codes_row_stride >= 0 && s.codes_row_stride % 8 == 0 &&
             (s.norm.rows <= 1 || s.codes_row_stride >= s.norm.n),
             "%s: codes must be 8-byte aligned, with a row stride that is a non-negative multiple of 8 and (rows > 1) at least n", op);
    const View out[] = {
        view_rows("codes", s.codes, s.norm.rows, s.codes_row_stride, s.norm.n, 1),
        quant_scales_view(s.scales, s.mode, s.norm.rows, s.norm.n),
    };
    return add_norm_check(s.norm, op, out, 2);
}

// fa_act_mul_quant's argument rules
static int act_mul_quant_check(const fa_act_mul_quant_params& s) {
    const char* op = "act_mul_quant";
    FA_CHECK(s.gate, "%s: gate must not be NULL", op);
    FA_CHECK(s.reserved0 == 0 && s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0,
             "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(check_io_dtype(op, s.dtype, "dtype"));
    FA_CHECK(s.activation >= FA_ACT_SILU && s.activation <= FA_ACT_RELU2, "%s: unknown activation %d", op, s.activation);
    FA_TRY(quant_n_check(op, s.n));
    FA_TRY(quant_rule_check(op, s.mode, s.has_scale_ub, s.scale, s.scale_ub, s.codes, s.scales, s.n));
    FA_CHECK(s.rows >= 0, "%s: rows must be non-negative", op);
    FA_CHECK(act_stride_ok(s.gate, s.gate_row_stride, s.rows, s.n) && act_stride_ok(s.up, s.up_row_stride, s.rows, s.n) &&
             act_stride_ok(s.codes, s.codes_row_stride, s.rows, s.n), "%s: row strides must be non-negative and (rows > 1) at least n", op);
    FA_CHECK(((addr(s.gate) | addr(s.up)) & 1) == 0, "%s: gate / up must be aligned to their element", op);
    if (s.rows > 0x7fffffffLL) return fail(FA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 rows in one launch", op);
    const View in[] = {
        view_rows("gate", s.gate, s.rows, s.gate_row_stride, s.n, 2),
        view_rows("up", s.up, s.rows, s.up_row_stride, s.n, 2),
    };
    const View out[] = {
        view_rows("codes", s.codes, s.rows, s.codes_row_stride, s.n, 1),
        quant_scales_view(s.scales, s.mode, s.rows, s.n),
    };
    return check_overlaps(op, out, 2, in, 2, true);
}

// ---- fa_moe_*
template <typename P>
static bool moe_reserved_zero(const P& s) { return s.reserved[0] == 0 && s.reserved[1] == 0 && s.reserved[2] == 0 && s.reserved[3] == 0; }

// the sizes every fa_moe_* op shares; slots = tokens * top_k fits 31 bits afterwards
static int moe_sizes_check(const char* op, int64_t tokens, int num_experts, int top_k) {
    FA_CHECK(tokens >= 0, "%s: tokens must be non-negative", op);
    if (num_experts < 2 || num_experts > fa::MOE_MAX_EXPERTS)
        return fail(FA_ERR_UNSUPPORTED, "%s: num_experts must be in [2, %d], got %d", op, fa::MOE_MAX_EXPERTS, num_experts);
    const int kmax = num_experts < fa::MOE_MAX_TOPK ? num_experts : fa::MOE_MAX_TOPK;
    if (top_k < 1 || top_k > kmax)
        return fail(FA_ERR_UNSUPPORTED, "%s: top_k must be in [1, min(num_experts, %d)] = [1, %d], got %d", op, fa::MOE_MAX_TOPK, kmax, top_k);
    if (tokens > 0x7fffffffLL / top_k)
        return fail(FA_ERR_UNSUPPORTED, "%s: tokens x top_k must stay below 2^31", op);
    return FA_OK;
}

// the router's own fields: dtype, scoring, scale, the row strides
static int moe_route_common_check(const char* op, int dtype, int scoring, int renormalize, float scale) {
    FA_CHECK(dtype == FA_FP16 || dtype == FA_BF16 || dtype == FA_FP32, "%s: dtype must be fp16, bf16 or fp32", op);
    FA_CHECK(scoring == FA_MOE_SOFTMAX || scoring == FA_MOE_SIGMOID, "%s: unknown scoring %d", op, scoring);
    FA_CHECK(renormalize == 0 || renormalize == 1, "%s: renormalize must be 0 or 1", op);
    FA_CHECK(scale >= -3.402823466e38f && scale <= 3.402823466e38f, "%s: scale must be finite", op);
    return FA_OK;
}
static bool moe_stride_ok(int64_t rs, int64_t rows, int n) { return rs >= 0 && (rows <= 1 || rs >= n); }

static int moe_route_check(const fa_moe_route_params& s) {
    const char* op = "moe_route";
    FA_CHECK(moe_reserved_zero(s), "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(moe_sizes_check(op, s.tokens, s.num_experts, s.top_k));
    FA_TRY(moe_route_common_check(op, s.dtype, s.scoring, s.renormalize, s.scale));
    FA_CHECK(s.scoring == FA_MOE_SIGMOID || !s.bias, "%s: bias goes with sigmoid scoring", op);
    if (s.tokens == 0) return FA_OK;
    FA_CHECK(s.logits && s.weights && s.ids, "%s: logits, weights and ids must not be NULL", op);
    FA_CHECK(moe_stride_ok(s.logits_row_stride, s.tokens, s.num_experts), "%s: logits_row_stride must be non-negative and (tokens > 1) at least num_experts", op);
    const int esize = s.dtype == FA_FP32 ? 4 : 2;
    FA_CHECK((addr(s.logits) & (esize - 1)) == 0 && ((addr(s.bias) | addr(s.weights) | addr(s.ids)) & 3) == 0,
             "%s: logits must be aligned to their element, bias / weights / ids to 4 bytes", op);
    const View in[] = {
        view_rows("logits", s.logits, s.tokens, s.logits_row_stride, s.num_experts, esize),
        view_flat("bias", s.bias, (uint64_t)s.num_experts * 4),
    };
    const View out[] = {
        view_flat("weights", s.weights, (uint64_t)s.tokens * s.top_k * 4),
        view_flat("ids", s.ids, (uint64_t)s.tokens * s.top_k * 4),
    };
    return check_overlaps(op, out, 2, in, 2, true, nullptr, 0);
}

static int moe_route_bwd_check(const fa_moe_route_bwd_params& s) {
    const char* op = "moe_route_bwd";
    FA_CHECK(moe_reserved_zero(s), "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(moe_sizes_check(op, s.tokens, s.num_experts, s.top_k));
    FA_TRY(moe_route_common_check(op, s.dtype, s.scoring, s.renormalize, s.scale));
    if (s.tokens == 0) return FA_OK;
    FA_CHECK(s.dweights && s.logits && s.ids && s.dlogits, "%s: dweights, logits, ids and dlogits must not be NULL", op);
    FA_CHECK(moe_stride_ok(s.logits_row_stride, s.tokens, s.num_experts) && moe_stride_ok(s.dlogits_row_stride, s.tokens, s.num_experts),
             "%s: row strides must be non-negative and (tokens > 1) at least num_experts", op);
    FA_CHECK(s.tokens <= 1 || s.dlogits_row_stride >= s.num_experts, "%s: dlogits rows must not overlap", op);
    const int esize = s.dtype == FA_FP32 ? 4 : 2;
    FA_CHECK(((addr(s.logits) | addr(s.dlogits)) & (esize - 1)) == 0 && ((addr(s.dweights) | addr(s.ids)) & 3) == 0,
             "%s: logits / dlogits must be aligned to their element, dweights / ids to 4 bytes", op);
    const View in[] = {
        view_rows("logits", s.logits, s.tokens, s.logits_row_stride, s.num_experts, esize),
        view_flat("dweights", s.dweights, (uint64_t)s.tokens * s.top_k * 4),
        view_flat("ids", s.ids, (uint64_t)s.tokens * s.top_k * 4),
    };
    const View out = view_rows("dlogits", s.dlogits, s.tokens, s.dlogits_row_stride, s.num_experts, esize);
    return check_overlaps(op, &out, 1, in, 3, false, nullptr, 0);
}

// query: the workspace is not looked at
static int moe_sort_check(const fa_moe_sort_params& s, bool query) {
    const char* op = "moe_sort";
    FA_CHECK(s.reserved0 == 0 && moe_reserved_zero(s), "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(moe_sizes_check(op, s.tokens, s.num_experts, s.top_k));
    if (s.align < 1 || s.align > fa::MOE_MAX_ALIGN)
        return fail(FA_ERR_UNSUPPORTED, "%s: align must be in [1, %d], got %d", op, fa::MOE_MAX_ALIGN, s.align);
    const int64_t slots = s.tokens * s.top_k, mmax = slots + (int64_t)s.num_experts * (s.align - 1);
    if (mmax > 0x7fffffffLL)
        return fail(FA_ERR_UNSUPPORTED, "%s: tokens x top_k + num_experts x (align - 1) must stay below 2^31", op);
    if (query) return FA_OK;
    FA_CHECK(s.expert_offsets && (slots == 0 || (s.ids && s.pos)) && (mmax == 0 || s.sorted_slot),
             "%s: ids, sorted_slot, pos and expert_offsets must not be NULL", op);
    FA_CHECK(((addr(s.ids) | addr(s.sorted_slot) | addr(s.pos) | addr(s.expert_offsets) | addr(s.workspace)) & 3) == 0,
             "%s: ids, sorted_slot, pos, expert_offsets and workspace must be 4-byte aligned", op);
    const size_t need = fa::moe_sort_plan(slots, s.num_experts).workspace_bytes;
    FA_CHECK(s.workspace && s.workspace_bytes >= need, "%s: workspace too small (%zu bytes, need %zu)", op, s.workspace ? s.workspace_bytes : (size_t)0, need);
    const View in[] = {view_flat("ids", s.ids, (uint64_t)slots * 4)};
    const View out[] = {
        view_flat("sorted_slot", s.sorted_slot, (uint64_t)mmax * 4),
        view_flat("pos", s.pos, (uint64_t)slots * 4),
        view_flat("expert_offsets", s.expert_offsets, (uint64_t)(s.num_experts + 1) * 4),
        view_flat("workspace", s.workspace, need),
    };
    return check_overlaps(op, out, 4, in, 1, true, nullptr, 0);
}

// the [rows, n] 16-bit tensors of permute / combine: n, dtype, 16-byte pieces
static int moe_hidden_check(const char* op, int n, int dtype) {
    FA_TRY(check_io_dtype(op, dtype, "dtype"));
    if (n < 8 || n > fa::MOE_MAX_N || n % 8 != 0)
        return fail(FA_ERR_UNSUPPORTED, "%s: n must be a multiple of 8 in [8, %d], got %d", op, fa::MOE_MAX_N, n);
    return FA_OK;
}
static bool moe_rows_ok(const void* p, int64_t rs, int64_t rows, int n) {
    return !p || ((addr(p) & 15) == 0 && rs >= 0 && rs % 8 == 0 && (rows <= 1 || rs >= n));
}
static const char* const kMoeRowsRule = "16-byte aligned with row strides that are multiples of 8 and (rows > 1) at least n";

static int moe_permute_check(const fa_moe_permute_params& s) {
    const char* op = "moe_permute";
    FA_CHECK(s.reserved0 == 0 && moe_reserved_zero(s), "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_CHECK(s.tokens >= 0 && s.rows >= 0, "%s: tokens and rows must be non-negative", op);
    if (s.top_k < 1 || s.top_k > fa::MOE_MAX_TOPK)
        return fail(FA_ERR_UNSUPPORTED, "%s: top_k must be in [1, %d], got %d", op, fa::MOE_MAX_TOPK, s.top_k);
    if (s.tokens > 0x7fffffffLL / s.top_k || s.rows > 0x7fffffffLL)
        return fail(FA_ERR_UNSUPPORTED, "%s: tokens x top_k and rows must stay below 2^31", op);
    FA_TRY(moe_hidden_check(op, s.n, s.dtype));
    if (s.rows == 0) return FA_OK;
    FA_CHECK(s.out && (s.tokens == 0 || s.x), "%s: x and out must not be NULL", op);
    FA_CHECK(moe_rows_ok(s.x, s.x_row_stride, s.tokens, s.n) && moe_rows_ok(s.out, s.out_row_stride, s.rows, s.n), "%s: x and out must be %s", op, kMoeRowsRule);
    FA_CHECK(s.rows <= 1 || s.out_row_stride >= s.n, "%s: out rows must not overlap", op);
    FA_CHECK(((addr(s.sorted_slot) | addr(s.slot_scale)) & 3) == 0, "%s: sorted_slot and slot_scale must be 4-byte aligned", op);
    const View in[] = {
        view_rows("x", s.x, s.tokens, s.x_row_stride, s.n, 2),
        view_flat("sorted_slot", s.sorted_slot, (uint64_t)s.rows * 4),
        view_flat("slot_scale", s.slot_scale, (uint64_t)s.tokens * s.top_k * 4),
    };
    const View out = view_rows("out", s.out, s.rows, s.out_row_stride, s.n, 2);
    return check_overlaps(op, &out, 1, in, 3, false, nullptr, 0);
}

// the shape arguments fa_moe_gemm, fa_moe_gemm_wgrad and their plans share
static int moe_gemm_dims_check(const char* op, int64_t rows, int n, int k, int num_experts, int layout, int dtype) {
    FA_CHECK(rows >= 0, "%s: rows must be non-negative", op);
    FA_TRY(check_io_dtype(op, dtype, "dtype"));
    FA_CHECK(layout == FA_MOE_W_NK || layout == FA_MOE_W_KN, "%s: layout must be FA_MOE_W_NK or FA_MOE_W_KN, got %d", op, layout);
    if (num_experts < 2 || num_experts > fa::MOE_MAX_EXPERTS)
        return fail(FA_ERR_UNSUPPORTED, "%s: num_experts must be in [2, %d], got %d", op, fa::MOE_MAX_EXPERTS, num_experts);
    if (n < 8 || n > fa::MOE_GEMM_MAX_N || n % 8 != 0)
        return fail(FA_ERR_UNSUPPORTED, "%s: n must be a multiple of 8 in [8, %d], got %d", op, fa::MOE_GEMM_MAX_N, n);
    if (k < 8 || k > fa::MOE_GEMM_MAX_K || k % 8 != 0)
        return fail(FA_ERR_UNSUPPORTED, "%s: k must be a multiple of 8 in [8, %d], got %d", op, fa::MOE_GEMM_MAX_K, k);
    if (rows > 0x7fffffffLL) return fail(FA_ERR_UNSUPPORTED, "%s: rows must stay below 2^31", op);
    return FA_OK;
}

// the same and the forward's grid bound
static int moe_gemm_shape_check(const char* op, int64_t rows, int n, int k, int num_experts, int layout, int dtype) {
    FA_TRY(moe_gemm_dims_check(op, rows, n, k, num_experts, layout, dtype));
    if (fa::moe_gemm_plan(rows, n, k, num_experts, layout, dtype).grid_m >= (1 << 24))
        return fail(FA_ERR_UNSUPPORTED, "%s: rows = %lld needs more row tiles than one launch has", op, (long long)rows);
    return FA_OK;
}

static int moe_gemm_check(const fa_moe_gemm_params& s) {
    const char* op = "moe_gemm";
    FA_CHECK(s.reserved0 == 0 && moe_reserved_zero(s), "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(moe_gemm_shape_check(op, s.rows, s.n, s.k, s.num_experts, s.layout, s.dtype));
    const bool gather = s.sorted_slot != nullptr;
    if (gather) {
        FA_CHECK(s.tokens >= 0, "%s: tokens must be non-negative", op);
        if (s.top_k < 1 || s.top_k > fa::MOE_MAX_TOPK)
            return fail(FA_ERR_UNSUPPORTED, "%s: top_k must be in [1, %d], got %d", op, fa::MOE_MAX_TOPK, s.top_k);
        if (s.tokens > 0x7fffffffLL / s.top_k) return fail(FA_ERR_UNSUPPORTED, "%s: tokens x top_k must stay below 2^31", op);
    }
    if (s.w_expert_stride < (int64_t)s.n * s.k || s.w_expert_stride % 8 != 0)
        return fail(FA_ERR_UNSUPPORTED, "%s: w_expert_stride must be a multiple of 8 and at least n x k = %lld, got %lld", op,
                    (long long)s.n * s.k, (long long)s.w_expert_stride);
    if (s.x_row_stride < 0 || s.x_row_stride % 8 != 0 || s.x_row_stride > fa::MOE_GEMM_MAX_ROW_STRIDE)
        return fail(FA_ERR_UNSUPPORTED, "%s: x_row_stride must be a multiple of 8 in [0, 2^22], got %lld", op, (long long)s.x_row_stride);
    if (s.out_row_stride < 0 || s.out_row_stride % 8 != 0 || s.out_row_stride > fa::MOE_GEMM_MAX_ROW_STRIDE)
        return fail(FA_ERR_UNSUPPORTED, "%s: out_row_stride must be a multiple of 8 in [0, 2^22], got %lld", op, (long long)s.out_row_stride);
    if (s.bias && s.bias_dtype != s.dtype && s.bias_dtype != FA_FP32)
        return fail(FA_ERR_UNSUPPORTED, "%s: bias_dtype must be dtype or fp32", op);
    if (s.rows == 0) return FA_OK;
    const int64_t x_rows = gather ? s.tokens : s.rows;
    FA_CHECK(s.out && s.w && s.expert_offsets && (x_rows == 0 || s.x), "%s: x, w, expert_offsets and out must not be NULL", op);
    FA_CHECK(s.rows <= 1 || s.out_row_stride >= s.n, "%s: out rows must not overlap (out_row_stride >= n)", op);
    FA_CHECK(x_rows <= 1 || s.x_row_stride >= s.k, "%s: x_row_stride must be at least k", op);
    FA_CHECK(((addr(s.x) | addr(s.w) | addr(s.out)) & 15) == 0, "%s: x, w and out must be 16-byte aligned", op);
    FA_CHECK(((addr(s.expert_offsets) | addr(s.sorted_slot)) & 3) == 0 && (addr(s.bias) & (s.bias_dtype == FA_FP32 ? 3 : 1)) == 0,
             "%s: expert_offsets, sorted_slot and bias must be aligned to their elements", op);
    const View in[] = {
        view_rows("x", s.x, x_rows, s.x_row_stride, s.k, 2),
        view_rows("w", s.w, s.num_experts, s.w_expert_stride, (int64_t)s.n * s.k, 2),
        view_flat("bias", s.bias, (uint64_t)s.num_experts * s.n * (s.bias_dtype == FA_FP32 ? 4 : 2)),
        view_flat("expert_offsets", s.expert_offsets, (uint64_t)(s.num_experts + 1) * 4),
        view_flat("sorted_slot", s.sorted_slot, (uint64_t)s.rows * 4),
    };
    const View out = view_rows("out", s.out, s.rows, s.out_row_stride, s.n, 2);
    return check_overlaps(op, &out, 1, in, 5, false, nullptr, 0);
}

static int moe_gemm_wgrad_check(const fa_moe_gemm_wgrad_params& s) {
    const char* op = "moe_gemm_wgrad";
    FA_CHECK(s.reserved0 == 0 && moe_reserved_zero(s), "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_TRY(moe_gemm_dims_check(op, s.rows, s.n, s.k, s.num_experts, s.layout, s.dtype));
    const bool gather = s.sorted_slot != nullptr;
    if (gather) {
        FA_CHECK(s.tokens >= 0, "%s: tokens must be non-negative", op);
        if (s.top_k < 1 || s.top_k > fa::MOE_MAX_TOPK)
            return fail(FA_ERR_UNSUPPORTED, "%s: top_k must be in [1, %d], got %d", op, fa::MOE_MAX_TOPK, s.top_k);
        if (s.tokens > 0x7fffffffLL / s.top_k) return fail(FA_ERR_UNSUPPORTED, "%s: tokens x top_k must stay below 2^31", op);
    }
    if (s.dw_dtype != s.dtype && s.dw_dtype != FA_FP32) return fail(FA_ERR_UNSUPPORTED, "%s: dw_dtype must be dtype or fp32", op);
    if (s.accumulate && s.dw_dtype != FA_FP32) return fail(FA_ERR_UNSUPPORTED, "%s: accumulate needs an fp32 dw (dw_dtype)", op);
    if (s.dbias && s.dbias_dtype != s.dtype && s.dbias_dtype != FA_FP32)
        return fail(FA_ERR_UNSUPPORTED, "%s: dbias_dtype must be dtype or fp32", op);
    if (s.dw && (s.dw_expert_stride < (int64_t)s.n * s.k || s.dw_expert_stride % 8 != 0))
        return fail(FA_ERR_UNSUPPORTED, "%s: dw_expert_stride must be a multiple of 8 and at least n x k = %lld, got %lld", op,
                    (long long)s.n * s.k, (long long)s.dw_expert_stride);
    if (s.dy_row_stride < 0 || s.dy_row_stride % 8 != 0 || s.dy_row_stride > fa::MOE_GEMM_MAX_ROW_STRIDE)
        return fail(FA_ERR_UNSUPPORTED, "%s: dy_row_stride must be a multiple of 8 in [0, 2^22], got %lld", op, (long long)s.dy_row_stride);
    if (s.x_row_stride < 0 || s.x_row_stride % 8 != 0 || s.x_row_stride > fa::MOE_GEMM_MAX_ROW_STRIDE)
        return fail(FA_ERR_UNSUPPORTED, "%s: x_row_stride must be a multiple of 8 in [0, 2^22], got %lld", op, (long long)s.x_row_stride);
    FA_CHECK(s.expert_offsets, "%s: expert_offsets must not be NULL", op);
    const int64_t x_rows = gather ? s.tokens : s.rows;
    FA_CHECK((s.rows == 0 || s.dy) && (s.rows == 0 || !s.dw || x_rows == 0 || s.x), "%s: dy and x must not be NULL", op);
    FA_CHECK(s.rows <= 1 || s.dy_row_stride >= s.n, "%s: dy_row_stride must be at least n", op);
    FA_CHECK(x_rows <= 1 || s.x_row_stride >= s.k, "%s: x_row_stride must be at least k", op);
    FA_CHECK(((addr(s.dy) | addr(s.x) | addr(s.dw)) & 15) == 0, "%s: dy, x and dw must be 16-byte aligned", op);
    FA_CHECK(((addr(s.expert_offsets) | addr(s.sorted_slot)) & 3) == 0 && (addr(s.dbias) & (s.dbias_dtype == FA_FP32 ? 3 : 1)) == 0,
             "%s: expert_offsets, sorted_slot and dbias must be aligned to their elements", op);
    const int wsz = s.dw_dtype == FA_FP32 ? 4 : 2;
    const View in[] = {
        view_rows("dy", s.dy, s.rows, s.dy_row_stride, s.n, 2),
        view_rows("x", s.x, x_rows, s.x_row_stride, s.k, 2),
        view_flat("expert_offsets", s.expert_offsets, (uint64_t)(s.num_experts + 1) * 4),
        view_flat("sorted_slot", s.sorted_slot, (uint64_t)s.rows * 4),
    };
    const View out[] = {
        view_rows("dw", s.dw, s.num_experts, s.dw_expert_stride, (int64_t)s.n * s.k, wsz),
        view_flat("dbias", s.dbias, (uint64_t)s.num_experts * s.n * (s.dbias_dtype == FA_FP32 ? 4 : 2)),
    };
    return check_overlaps(op, out, 2, in, 4, true, nullptr, 0);
}

static int moe_combine_check(const fa_moe_combine_params& s) {
    const char* op = "moe_combine";
    FA_CHECK(s.reserved0 == 0 && moe_reserved_zero(s), "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_CHECK(s.tokens >= 0 && s.rows >= 0, "%s: tokens and rows must be non-negative", op);
    if (s.top_k < 1 || s.top_k > fa::MOE_MAX_TOPK)
        return fail(FA_ERR_UNSUPPORTED, "%s: top_k must be in [1, %d], got %d", op, fa::MOE_MAX_TOPK, s.top_k);
    if (s.tokens > 0x7fffffffLL / s.top_k || s.rows > 0x7fffffffLL)
        return fail(FA_ERR_UNSUPPORTED, "%s: tokens x top_k and rows must stay below 2^31", op);
    FA_TRY(moe_hidden_check(op, s.n, s.dtype));
    if (s.tokens == 0) return FA_OK;
    FA_CHECK(s.out && s.pos && (s.rows == 0 || s.y), "%s: y, pos and out must not be NULL", op);
    FA_CHECK(moe_rows_ok(s.y, s.y_row_stride, s.rows, s.n) && moe_rows_ok(s.out, s.out_row_stride, s.tokens, s.n), "%s: y and out must be %s", op, kMoeRowsRule);
    FA_CHECK(((addr(s.pos) | addr(s.weights)) & 3) == 0, "%s: pos and weights must be 4-byte aligned", op);
    const View in[] = {
        view_rows("y", s.y, s.rows, s.y_row_stride, s.n, 2),
        view_flat("pos", s.pos, (uint64_t)s.tokens * s.top_k * 4),
        view_flat("weights", s.weights, (uint64_t)s.tokens * s.top_k * 4),
    };
    const View out = view_rows("out", s.out, s.tokens, s.out_row_stride, s.n, 2);
    return check_overlaps(op, &out, 1, in, 3, false, nullptr, 0);
}

static int moe_combine_bwd_check(const fa_moe_combine_bwd_params& s) {
    const char* op = "moe_combine_bwd";
    FA_CHECK(s.reserved0 == 0 && moe_reserved_zero(s), "%s: reserved fields must be 0 (zero-initialise the struct)", op);
    FA_CHECK(s.tokens >= 0 && s.rows >= 0, "%s: tokens and rows must be non-negative", op);
    if (s.top_k < 1 || s.top_k > fa::MOE_MAX_TOPK)
        return fail(FA_ERR_UNSUPPORTED, "%s: top_k must be in [1, %d], got %d", op, fa::MOE_MAX_TOPK, s.top_k);
    if (s.tokens > 0x7fffffffLL / s.top_k || s.rows > 0x7fffffffLL)
        return fail(FA_ERR_UNSUPPORTED, "%s: tokens x top_k and rows must stay below 2^31", op);
    FA_TRY(moe_hidden_check(op, s.n, s.dtype));
    if (!s.dy && !s.dw) return FA_OK;
    const bool live = s.tokens > 0;
    FA_CHECK(!live || (s.dout && s.pos), "%s: dout and pos must not be NULL", op);
    FA_CHECK(!s.dy || !live || s.weights, "%s: dy needs weights", op);
    FA_CHECK(!s.dw || !live || s.rows == 0 || s.y, "%s: dw needs y", op);
    FA_CHECK(moe_rows_ok(s.dout, s.dout_row_stride, s.tokens, s.n) && moe_rows_ok(s.y, s.y_row_stride, s.rows, s.n) &&
             moe_rows_ok(s.dy, s.dy_row_stride, s.rows, s.n), "%s: dout, y and dy must be %s", op, kMoeRowsRule);
    FA_CHECK(((addr(s.pos) | addr(s.weights) | addr(s.dw)) & 3) == 0, "%s: pos, weights and dw must be 4-byte aligned", op);
    const View in[] = {
        view_rows("dout", s.dout, s.tokens, s.dout_row_stride, s.n, 2),
        view_rows("y", s.dw ? s.y : nullptr, s.rows, s.y_row_stride, s.n, 2),
        view_flat("pos", s.pos, (uint64_t)s.tokens * s.top_k * 4),
        view_flat("weights", s.dy ? s.weights : nullptr, (uint64_t)s.tokens * s.top_k * 4),
    };
    const View out[] = {
        view_rows("dy", s.dy, s.rows, s.dy_row_stride, s.n, 2),
        view_flat("dw", s.dw, (uint64_t)s.tokens * s.top_k * 4),
    };
    return check_overlaps(op, out, 2, in, 4, true, nullptr, 0);
}


extern "C" {

int fa_rotary(const fa_rotary_params* r, void* stream) {
    FA_TRY(check_header(r, "fa_rotary_params"));
    bool empty;
    FA_TRY(rotary_check(*r, &empty));
    if (empty) return FA_OK;
    fa::launch_rotary(*r, static_cast<hipStream_t>(stream));
    return check_hip("fa_rotary launch");
}

int fa_kv_store(const fa_kv_store_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_kv_store_params"));
    fa_kv_store_params s = *sp;
    bool empty;
    FA_TRY(kv_store_check(s, &empty));
    if (empty) return FA_OK;
    fa::launch_kv_store(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_kv_store launch");
}

int fa_kv_gather(const fa_kv_gather_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_kv_gather_params"));
    fa_kv_gather_params s = *sp;
    bool empty;
    FA_TRY(kv_gather_check(s, &empty));
    if (empty) return FA_OK;
    fa::launch_kv_gather(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_kv_gather launch");
}

int fa_rope_store(const fa_rope_store_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_rope_store_params"));
    fa_rope_store_params s = *sp;
    bool empty;
    FA_TRY(rope_store_check(s, "rope_store", false, nullptr, 0, &empty));
    if (empty) return FA_OK;
    fa::launch_rope_store(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_rope_store launch");
}

int fa_qk_norm_rope_store(const fa_qk_norm_rope_store_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_qk_norm_rope_store_params"));
    fa_qk_norm_rope_store_params s = *sp;
    bool empty;
    FA_TRY(qk_norm_rope_store_check(s, &empty));
    if (empty) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_qk_norm_rope_store(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_qk_norm_rope_store launch");
}

size_t fa_qk_norm_rope_bwd_workspace_bytes(const fa_qk_norm_rope_bwd_params* sp) {
    if (!sp || sp->struct_size < sizeof(fa_qk_norm_rope_bwd_params)) return 0;
    fa_qk_norm_rope_bwd_params s = *sp;
    if (qk_norm_rope_bwd_check(s, true) != FA_OK) return 0;
    return fa::qk_norm_rope_bwd_workspace_bytes(s);
}

int fa_qk_norm_rope_bwd(const fa_qk_norm_rope_bwd_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_qk_norm_rope_bwd_params"));
    fa_qk_norm_rope_bwd_params s = *sp;
    FA_TRY(qk_norm_rope_bwd_check(s, false));
    const bool empty = s.total_rows == 0 || s.head_dim == 0 || (s.nheads_q == 0 && s.nheads_k == 0);
    if (empty && !s.dq_weight && !s.dk_weight) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_qk_norm_rope_bwd(s, static_cast<hipStream_t>(stream));      // (an empty problem: a wanted dw is set to zeros, no kernel)
    return check_hip("fa_qk_norm_rope_bwd launch");
}

int fa_add_norm(const fa_add_norm_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_add_norm_params"));
    fa_add_norm_params s = *sp;
    FA_TRY(add_norm_check(s));
    if (s.rows == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_add_norm(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_add_norm launch");
}

size_t fa_add_norm_bwd_workspace_bytes(const fa_add_norm_bwd_params* sp) {
    if (!sp || sp->struct_size < sizeof(fa_add_norm_bwd_params)) return 0;
    if (add_norm_bwd_check(*sp, true) != FA_OK) return 0;
    return fa::add_norm_bwd_workspace_bytes(*sp);
}

int fa_add_norm_bwd(const fa_add_norm_bwd_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_add_norm_bwd_params"));
    fa_add_norm_bwd_params s = *sp;
    FA_TRY(add_norm_bwd_check(s, false));
    if (!s.dx && !s.dres && !s.dweight && !s.dbias) return FA_OK;
    if (s.rows == 0 && !s.dweight && !s.dbias) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_add_norm_bwd(s, static_cast<hipStream_t>(stream));          // (rows == 0: a wanted dweight / dbias is set to zeros, no kernel)
    return check_hip("fa_add_norm_bwd launch");
}

size_t fa_cross_entropy_workspace_bytes(const fa_cross_entropy_params* sp) {
    if (!sp || sp->struct_size < sizeof(fa_cross_entropy_params)) return 0;
    if (cross_entropy_check(*sp, true) != FA_OK) return 0;
    return fa::cross_entropy_workspace_bytes(sp->rows, sp->vocab, sp->dtype);
}

int fa_cross_entropy(const fa_cross_entropy_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_cross_entropy_params"));
    fa_cross_entropy_params s = *sp;
    FA_TRY(cross_entropy_check(s, false));
    if (s.rows == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_cross_entropy(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_cross_entropy launch");
}

size_t fa_sample_workspace_bytes(const fa_sample_params* sp) {
    if (!sp || sp->struct_size < sizeof(fa_sample_params)) return 0;
    if (sample_check(*sp, true) != FA_OK) return 0;
    return fa::sample_workspace_bytes(sp->rows, sp->vocab, sp->dtype);
}

int fa_sample(const fa_sample_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_sample_params"));
    fa_sample_params s = *sp;
    FA_TRY(sample_check(s, false));
    if (s.rows == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_sample(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_sample launch");
}

size_t fa_spec_accept_workspace_bytes(const fa_spec_accept_params* sp) {
    if (!sp || sp->struct_size < sizeof(fa_spec_accept_params)) return 0;
    if (spec_accept_check(*sp, true) != FA_OK) return 0;
    return fa::spec_accept_workspace_bytes(sp->batch * sp->nodes, sp->vocab);
}

int fa_spec_accept(const fa_spec_accept_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_spec_accept_params"));
    fa_spec_accept_params s = *sp;
    FA_TRY(spec_accept_check(s, false));
    if (s.batch == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_spec_accept(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_spec_accept launch");
}

int fa_spec_walk(const fa_spec_walk_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_spec_walk_params"));
    fa_spec_walk_params s = *sp;
    FA_TRY(spec_walk_check(s));
    if (s.batch == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_spec_walk(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_spec_walk launch");
}

int fa_cross_entropy_bwd(const fa_cross_entropy_bwd_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_cross_entropy_bwd_params"));
    fa_cross_entropy_bwd_params s = *sp;
    FA_TRY(cross_entropy_bwd_check(s));
    if (s.rows == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_cross_entropy_bwd(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_cross_entropy_bwd launch");
}

int fa_act_mul_plan(int64_t rows, int32_t n, int64_t* run_columns, int64_t* items, int64_t* grid) {
    FA_TRY(act_mul_common_check("act_mul_plan", FA_BF16, FA_ACT_SILU, n, rows));
    const fa::ActPlan pl = fa::act_plan(rows, n);
    if (run_columns) *run_columns = 8 * (int64_t)pl.chunk_pieces;
    if (items) *items = pl.items;
    if (grid) *grid = pl.grid;
    return FA_OK;
}

int fa_act_mul(const fa_act_mul_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_act_mul_params"));
    fa_act_mul_params s = *sp;
    FA_TRY(act_mul_check(s));
    if (s.rows == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_act_mul(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_act_mul launch");
}

int fa_act_mul_bwd(const fa_act_mul_bwd_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_act_mul_bwd_params"));
    fa_act_mul_bwd_params s = *sp;
    FA_TRY(act_mul_bwd_check(s));
    if (s.rows == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_act_mul_bwd(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_act_mul_bwd launch");
}

int fa_quant_fp8(const fa_quant_fp8_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_quant_fp8_params"));
    fa_quant_fp8_params s = *sp;
    FA_TRY(quant_fp8_check(s));
    if (s.rows == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_quant_fp8(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_quant_fp8 launch");
}

int fa_add_norm_quant(const fa_add_norm_quant_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_add_norm_quant_params"));
    fa_add_norm_quant_params s = *sp;
    FA_TRY(add_norm_quant_check(s));
    if (s.norm.rows == 0) return FA_OK;
    s.struct_size = sizeof(s);
    s.norm.struct_size = sizeof(s.norm);
    fa::launch_add_norm_quant(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_add_norm_quant launch");
}

int fa_act_mul_quant(const fa_act_mul_quant_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_act_mul_quant_params"));
    fa_act_mul_quant_params s = *sp;
    FA_TRY(act_mul_quant_check(s));
    if (s.rows == 0) return FA_OK;
    s.struct_size = sizeof(s);
    fa::launch_act_mul_quant(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_act_mul_quant launch");
}

int fa_moe_route(const fa_moe_route_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_moe_route_params"));
    fa_moe_route_params s = *sp;
    FA_TRY(moe_route_check(s));
    if (s.tokens == 0) return FA_OK;
    fa::launch_moe_route(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_moe_route launch");
}

int fa_moe_route_bwd(const fa_moe_route_bwd_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_moe_route_bwd_params"));
    fa_moe_route_bwd_params s = *sp;
    FA_TRY(moe_route_bwd_check(s));
    if (s.tokens == 0) return FA_OK;
    fa::launch_moe_route_bwd(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_moe_route_bwd launch");
}

size_t fa_moe_sort_workspace_bytes(const fa_moe_sort_params* sp) {
    if (!sp || sp->struct_size < sizeof(fa_moe_sort_params)) return 0;
    if (moe_sort_check(*sp, true) != FA_OK) return 0;
    return fa::moe_sort_plan(sp->tokens * sp->top_k, sp->num_experts).workspace_bytes;
}

int fa_moe_sort_plan(int64_t slots, int32_t num_experts, int64_t* chunk_slots, int64_t* chunks, int64_t* workspace_bytes) {
    FA_CHECK(slots >= 0, "moe_sort_plan: slots must be non-negative");
    if (slots > 0x7fffffffLL) return fail(FA_ERR_UNSUPPORTED, "moe_sort_plan: slots must stay below 2^31");
    if (num_experts < 2 || num_experts > fa::MOE_MAX_EXPERTS)
        return fail(FA_ERR_UNSUPPORTED, "moe_sort_plan: num_experts must be in [2, %d], got %d", fa::MOE_MAX_EXPERTS, num_experts);
    const fa::MoeSortPlan pl = fa::moe_sort_plan(slots, num_experts);
    if (chunk_slots) *chunk_slots = pl.chunk;
    if (chunks) *chunks = pl.chunks;
    if (workspace_bytes) *workspace_bytes = (int64_t)pl.workspace_bytes;
    return FA_OK;
}

int fa_moe_sort(const fa_moe_sort_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_moe_sort_params"));
    fa_moe_sort_params s = *sp;
    FA_TRY(moe_sort_check(s, false));
    fa::launch_moe_sort(s, static_cast<hipStream_t>(stream));   // (tokens == 0: the offsets and the padding are still written)
    return check_hip("fa_moe_sort launch");
}

int fa_moe_permute(const fa_moe_permute_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_moe_permute_params"));
    fa_moe_permute_params s = *sp;
    FA_TRY(moe_permute_check(s));
    if (s.rows == 0) return FA_OK;
    fa::launch_moe_permute(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_moe_permute launch");
}

int fa_moe_combine(const fa_moe_combine_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_moe_combine_params"));
    fa_moe_combine_params s = *sp;
    FA_TRY(moe_combine_check(s));
    if (s.tokens == 0) return FA_OK;
    fa::launch_moe_combine(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_moe_combine launch");
}

int fa_moe_combine_bwd(const fa_moe_combine_bwd_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_moe_combine_bwd_params"));
    fa_moe_combine_bwd_params s = *sp;
    FA_TRY(moe_combine_bwd_check(s));
    if ((!s.dy || s.rows == 0) && (!s.dw || s.tokens == 0)) return FA_OK;
    if (s.rows == 0) s.dy = nullptr;
    fa::launch_moe_combine_bwd(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_moe_combine_bwd launch");
}

int fa_moe_gemm_plan(int64_t rows, int32_t n, int32_t k, int32_t num_experts, int32_t layout, int32_t dtype,
                     int32_t* block_m, int32_t* block_n, int32_t* block_k, int64_t* grid_m, int64_t* grid_n) {
    FA_TRY(moe_gemm_shape_check("moe_gemm_plan", rows, n, k, num_experts, layout, dtype));
    const fa::MoeGemmPlan pl = fa::moe_gemm_plan(rows, n, k, num_experts, layout, dtype);
    if (block_m) *block_m = pl.bm;
    if (block_n) *block_n = pl.bn;
    if (block_k) *block_k = pl.bk;
    if (grid_m) *grid_m = pl.grid_m;
    if (grid_n) *grid_n = pl.grid_n;
    return FA_OK;
}

int fa_moe_gemm(const fa_moe_gemm_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_moe_gemm_params"));
    fa_moe_gemm_params s = *sp;
    FA_TRY(moe_gemm_check(s));
    if (s.rows == 0) return FA_OK;
    if (!s.sorted_slot) s.tokens = s.rows, s.top_k = 1;
    fa::launch_moe_gemm(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_moe_gemm launch");
}

int fa_moe_gemm_wgrad_plan(int32_t n, int32_t k, int32_t num_experts, int32_t layout, int32_t dtype,
                           int32_t* block_n, int32_t* block_k, int32_t* block_rows,
                           int64_t* grid_n, int64_t* grid_k, int64_t* grid_e) {
    FA_TRY(moe_gemm_dims_check("moe_gemm_wgrad_plan", 0, n, k, num_experts, layout, dtype));
    const fa::MoeWgradPlan pl = fa::moe_gemm_wgrad_plan(n, k, num_experts, layout, dtype);
    if (block_n) *block_n = pl.bn;
    if (block_k) *block_k = pl.bk;
    if (block_rows) *block_rows = pl.br;
    if (grid_n) *grid_n = pl.grid_n;
    if (grid_k) *grid_k = pl.grid_k;
    if (grid_e) *grid_e = pl.grid_e;
    return FA_OK;
}

int fa_moe_gemm_wgrad(const fa_moe_gemm_wgrad_params* sp, void* stream) {
    FA_TRY(check_header(sp, "fa_moe_gemm_wgrad_params"));
    fa_moe_gemm_wgrad_params s = *sp;
    FA_TRY(moe_gemm_wgrad_check(s));
    if (!s.dw && !s.dbias) return FA_OK;
    if (!s.sorted_slot) s.tokens = s.rows, s.top_k = 1;
    fa::launch_moe_gemm_wgrad(s, static_cast<hipStream_t>(stream));
    return check_hip("fa_moe_gemm_wgrad launch");
}

}  // extern "C"
