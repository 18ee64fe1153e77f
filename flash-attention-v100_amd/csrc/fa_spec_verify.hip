// fa_spec_verify.hip - speculative-decoding verification (fa_spec_accept, fa_spec_walk; include/fa_mi355.h): the rejection-sampling
// decision of every draft node from its target row of logits and its draft row of probabilities, and the one-wave walk that turns
// the decisions into emitted tokens and the accepted path.  The rules are in the header; in short, per node with e_j the masses
// of its target row and s their fixed-order sum (fa_mass.h: fa_sample's, because both ops call the same functions), d the draft
// token and q_j the draft probabilities as they are:
//     p_j = e_j * (1.0f / s)
//     accept = (uu * q_d < p_d);   r_j = min(max(p_j - q_j, 0), 1),  R_j = floor(r_j * 2^40)  (uint64),  R = sum R_j
//     R == 0: R_j := floor(e_j * 2^40);   recovered = the smallest index whose running sum of R_j exceeds min(floor(uu_r R), R - 1)
// Everything behind the R_j is INTEGER arithmetic: the sums do not depend on the order of addition.  No float atomics, no RNG, no
// host synchronisation: capturable.
// Launch plan, a function of vocab alone: a row is cut into C = ceil(vocab / MASS_CHUNK) chunks, one workgroup of 1024 lanes each (2
// pieces of 8 columns per lane; wave w of chunk c owns run c * 16 + w of the row: 1024 contiguous columns, lane l of it the pieces
// l and l + 64 of that run), and three kernels follow each other on the stream:
//     stats   nodes x C   the chunk's (m, s), first maximum and count of values above -inf over the target row -> one 32-byte
//                         partial in the workspace (plain stores)
//     mass    nodes x C   merges the node's partials in chunk order - every chunk gets the same (m, s) -, then the chunk's sum of
//                         R_j and of floor(e_j 2^40) -> two u64 in the workspace (plain stores)
//     final   nodes       the same merge, the totals, the accept test (two element loads), the chunk that holds rr, one sweep of
//                         that chunk: per-wave sums, then the one wave that holds rr walks its run with a shuffle scan
// Node 0, padding nodes, empty and greedy rows: the workgroups of `mass` leave at once and `final` writes the result from the
// partials alone.  No workgroup waits for another; the workspace needs no initialisation (everything read was written by the
// kernel in front).  A piece is one 16-byte load (fp32: two) where the row starts on a 16-byte boundary and the piece lies inside
// the row, element by element otherwise: the same values, never a column >= vocab.  No loop depends on the data.
#include "fa_mass.h"

namespace fa {
namespace spec {

// the residual of (p_j, q_j)
__device__ __forceinline__ float sp_r(float p, float q) {
    float r = p - q;
    r = r > 0.f ? r : 0.f;                                // (a NaN difference: 0)
    return r < 1.f ? r : 1.f;
}

struct SpSums { unsigned long long R, E; };
static_assert(sizeof(SpSums) == 16, "the workspace layout");

struct SpArgs {
    const void* x;                                        // target logits
    const void* q;                                        // draft probabilities
    const int32_t* draft_ids;
    const int32_t* parents;
    const float* u_accept;
    const float* u_recover;
    const float* temperature;
    int32_t* accept;
    int32_t* recovered;
    char* ws;
    int64_t x_rs, q_rs, par_bs, ws_per_row;
    int T, V, C;
    float temperature_value;
    __device__ __forceinline__ MassStat* stat(int64_t row) const { return reinterpret_cast<MassStat*>(ws + row * ws_per_row); }
    __device__ __forceinline__ SpSums* sums(int64_t row) const { return reinterpret_cast<SpSums*>(ws + row * ws_per_row + 32 * C); }
    __device__ __forceinline__ float temp(int64_t b) const { return temperature ? temperature[b] : temperature_value; }
};

// node `row` = (b, t): its parent, or -1 for node 0 and for a padding node
__device__ __forceinline__ int sp_parent(const SpArgs& a, int64_t row, int64_t& b) {
    b = row / a.T;
    const int t = (int)(row - b * a.T);
    if (t == 0) return -1;
    const int par = a.parents ? a.parents[b * a.par_bs + t] : t - 1;
    return par >= 0 && par < t ? par : -1;
}

template <typename T>
__global__ void __launch_bounds__(MASS_THREADS) spec_stats_kernel(const SpArgs a) {
    __shared__ float slotf[3 * MASS_WAVES];
    __shared__ uint32_t slot32[2 * MASS_WAVES];
    const int64_t row = (int64_t)blockIdx.x / a.C;
    const int chunk = (int)((int64_t)blockIdx.x - row * a.C);
    int64_t b;
    const int par = sp_parent(a, row, b);
    if (par < 0) return;
    const MassRow<T> r = mass_row_chunk<T>(a.x, (b * a.T + par) * a.x_rs, a.V, chunk);
    const MassStat o = mass_stats(r, mass_inv_t(a.temp(b)), slotf, slot32, threadIdx.x == 0);
    if (threadIdx.x == 0) a.stat(row)[chunk] = o;
}

// what a node's partials say: the same bits in every workgroup that asks
__device__ __forceinline__ MassNode sp_node(const SpArgs& a, int64_t row, int64_t b) {
    const MassStat stat = mass_merge(a.stat(row), a.C);
    return mass_node(stat, a.temp(b));
}

template <typename T, typename Q>
__global__ void __launch_bounds__(MASS_THREADS) spec_mass_kernel(const SpArgs a) {
    __shared__ uint64_t slot64[2 * MASS_WAVES];
    const int64_t row = (int64_t)blockIdx.x / a.C;
    const int chunk = (int)((int64_t)blockIdx.x - row * a.C);
    int64_t b;
    const int par = sp_parent(a, row, b);
    if (par < 0) return;
    const MassNode n = sp_node(a, row, b);
    if (n.empty || n.greedy) return;
    const float inv_s = 1.0f / n.st.s;
    const MassRow<T> xr = mass_row_chunk<T>(a.x, (b * a.T + par) * a.x_rs, a.V, chunk);
    const MassRow<Q> qr = mass_row_chunk<Q>(a.q, row * a.q_rs, a.V, chunk);
    uint64_t R = 0, E = 0;
    for (int i = 0; i < MASS_CHUNK_ITERS; ++i) {
        const int c = xr.col(i);
        if (c >= a.V) continue;
        float v[8], q[8];
        xr.values(c, v);
        qr.raw(c, 0.f, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float ee = mass_e(v[e], n.inv_t, n.m);
            E += mass_q(ee);
            R += mass_q(sp_r(ee * inv_s, q[e]));
        }
    }
    for (int m = 1; m < 64; m <<= 1) { R += shfl_xor64(R, m); E += shfl_xor64(E, m); }
    if (xr.lane == 0) { slot64[xr.wave] = R; slot64[MASS_WAVES + xr.wave] = E; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    SpSums o = {0, 0};
    for (int w = 0; w < MASS_WAVES; ++w) { o.R += slot64[w]; o.E += slot64[MASS_WAVES + w]; }
    a.sums(row)[chunk] = o;
}

template <typename T, typename Q>
__global__ void __launch_bounds__(MASS_THREADS) spec_final_kernel(const SpArgs a) {
    __shared__ uint64_t wtot[MASS_WAVES];
    __shared__ int found;
    const int64_t row = blockIdx.x;
    const bool lane0 = threadIdx.x == 0;
    int64_t b;
    const int par = sp_parent(a, row, b);
    if (par < 0) {
        if (lane0) { a.accept[row] = 0; a.recovered[row] = -1; }
        return;
    }
    const MassNode n = sp_node(a, row, b);
    const int d = a.draft_ids[row];
    if (n.empty || n.greedy) {
        if (lane0) {
            a.accept[row] = !n.empty && d == n.bi ? 1 : 0;
            a.recovered[row] = n.empty ? -1 : n.bi;
        }
        return;
    }
    const float inv_s = 1.0f / n.st.s;
    // ---- the totals; R == 0: the target's own masses
    const SpSums* sums = a.sums(row);
    uint64_t R = 0, E = 0;
    for (int c = 0; c < a.C; ++c) { R += sums[c].R; E += sums[c].E; }
    const bool own = R == 0;
    const uint64_t tot = own ? E : R;                     // (> 0: e_{j*} = 1)
    const uint64_t rr = mass_draw_target(a.u_recover[row], tot);
    uint64_t base = 0;
    int cstar = -1;
    for (int c = 0; c < a.C; ++c) {
        const uint64_t t = own ? sums[c].E : sums[c].R;
        if (cstar < 0) {
            if (base + t > rr) cstar = c;
            else base += t;
        }
    }
    const int chunk = cstar < 0 ? 0 : cstar;              // (no chunk holds rr: nothing is loaded below)
    const MassRow<T> xr = mass_row_chunk<T>(a.x, (b * a.T + par) * a.x_rs, a.V, chunk);
    const MassRow<Q> qr = mass_row_chunk<Q>(a.q, row * a.q_rs, a.V, chunk);
    // ---- accept
    if (lane0) {
        bool acc = false;
        if (d >= 0 && d < a.V) {
            const float pd = mass_e(mass_canon(RowIo<T>::load1(a.x, xr.rowoff + d)), n.inv_t, n.m) * inv_s;
            const float qd = RowIo<Q>::load1(a.q, qr.rowoff + d);
            const float ua = a.u_accept[row];
            const float uu = ua > 0.f ? ua : 0.f;
            acc = uu * qd < pd;
        }
        a.accept[row] = acc ? 1 : 0;
        found = n.bi;
    }
    // ---- the sweep of chunk cstar: the weights stay in registers for the walk
    uint64_t wv[MASS_CHUNK_ITERS][8];
    uint64_t ls[MASS_CHUNK_ITERS];
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < MASS_CHUNK_ITERS; ++i) {
        const int c = xr.col(i);
        ls[i] = 0;
        if (cstar >= 0 && c < a.V) {
            float v[8], q[8];
            xr.values(c, v);
            if (!own) qr.raw(c, 0.f, q);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ee = mass_e(v[e], n.inv_t, n.m);
                wv[i][e] = own ? mass_q(ee) : mass_q(sp_r(ee * inv_s, q[e]));
                ls[i] += wv[i][e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) wv[i][e] = 0;
        }
        s += ls[i];
    }
    for (int m = 1; m < 64; m <<= 1) s += shfl_xor64(s, m);
    if (xr.lane == 0) wtot[xr.wave] = s;
    __syncthreads();
    int wstar = -1;
    for (int w = 0; w < MASS_WAVES; ++w) {
        const uint64_t t = wtot[w];
        if (wstar < 0) {
            if (base + t > rr) wstar = w;
            else base += t;
        }
    }
    if (xr.wave == wstar) {
        uint64_t running = base;
#pragma unroll
        for (int i = 0; i < MASS_CHUNK_ITERS; ++i) mass_walk_step(wv[i], ls[i], running, rr, xr.col(i), xr.lane, found);
    }
    __syncthreads();
    if (lane0) a.recovered[row] = found;
}

// ---- the walk: one wave per request, lane t owns node t
struct SpWalkArgs {
    const int32_t* parents;
    const int32_t* draft_ids;
    const int32_t* target_ids;
    const int32_t* accept;
    const int32_t* recovered;
    int32_t* out_tokens;
    int32_t* num_out;
    int32_t* path_nodes;
    int64_t par_bs, tid_bs, tid_ns;
    int T;
};

__global__ void __launch_bounds__(64) spec_walk_kernel(const SpWalkArgs a) {
    const int64_t b = blockIdx.x;
    const int t = (int)threadIdx.x;
    const bool in = t < a.T;
    int par = -1, draft = -1, tgt = -1, acc = 0, rec = -1;
    if (in) {
        if (t >= 1) {
            par = a.parents ? a.parents[b * a.par_bs + t] : t - 1;
            if (par >= t) par = -1;                       // (a padding node; no cycle can arise)
            draft = a.draft_ids[b * a.T + t];
            if (a.accept) { acc = a.accept[b * a.T + t]; rec = a.recovered[b * a.T + t]; }
        }
        tgt = a.target_ids[b * a.tid_bs + (int64_t)t * a.tid_ns];
    }
    const bool child_ok = in && t >= 1 && par >= 0;
    int c = 0, n_out = 0, n_path = 1;
    int my_tok = -1, my_node = t == 0 ? 0 : -1;
    bool done = false;
    for (int step = 0; step < a.T; ++step) {              // (c, done, n_out and n_path are the same in every lane)
        if (done) break;
        int y;
        int next = -1;
        if (!a.accept) {
            y = __shfl(tgt, c);
            const unsigned long long kids = __ballot(child_ok && par == c && draft == y);
            if (y != -1 && kids) next = __ffsll((long long)kids) - 1;
        } else {
            const unsigned long long kids = __ballot(child_ok && par == c);
            if (!kids) {
                y = __shfl(tgt, c);
            } else {
                const int k = __ffsll((long long)kids) - 1;
                if (__shfl(acc, k) != 0) { y = __shfl(draft, k); next = k; }
                else y = __shfl(rec, k);
            }
        }
        if (t == n_out) my_tok = y;
        n_out += 1;
        if (next < 0) {
            done = true;
        } else {
            if (t == n_path) my_node = next;
            n_path += 1;
            c = next;
        }
    }
    if (in) {
        a.out_tokens[b * a.T + t] = t < n_out ? my_tok : -1;
        a.path_nodes[b * a.T + t] = t < n_path ? my_node : -1;
    }
    if (t == 0) a.num_out[b] = n_out;
}

}  // namespace spec

// ---- the host side: the launch plan is a function of vocab alone
int64_t spec_accept_chunks(int V) { return ((int64_t)V + MASS_CHUNK - 1) / MASS_CHUNK; }
static int64_t spec_ws_per_row(int V) { return (48 * spec_accept_chunks(V) + 63) / 64 * 64; }
size_t spec_accept_workspace_bytes(int64_t rows, int V) { return rows > 0 ? (size_t)rows * (size_t)spec_ws_per_row(V) : 0; }

template <typename T, typename Q>
static void launch_spec_accept_tq(const spec::SpArgs& a, int64_t rows, hipStream_t stream) {
    const dim3 gc((unsigned)(rows * a.C)), gr((unsigned)rows), b(MASS_THREADS);
    hipLaunchKernelGGL((spec::spec_stats_kernel<T>), gc, b, 0, stream, a);
    hipLaunchKernelGGL((spec::spec_mass_kernel<T, Q>), gc, b, 0, stream, a);
    hipLaunchKernelGGL((spec::spec_final_kernel<T, Q>), gr, b, 0, stream, a);
}
template <typename T>
static void launch_spec_accept_t(const spec::SpArgs& a, int64_t rows, int probs_dtype, hipStream_t stream) {
    if (probs_dtype == FA_BF16) launch_spec_accept_tq<T, bf16_tag>(a, rows, stream);
    else if (probs_dtype == FA_FP16) launch_spec_accept_tq<T, fp16_tag>(a, rows, stream);
    else launch_spec_accept_tq<T, fp32_tag>(a, rows, stream);
}

// The caller (fa_api.hip) has validated the block; batch > 0
void launch_spec_accept(const fa_spec_accept_params& s, hipStream_t stream) {
    spec::SpArgs a;
    a.x = s.target_logits; a.q = s.draft_probs; a.draft_ids = s.draft_ids; a.parents = s.parents;
    a.u_accept = s.u_accept; a.u_recover = s.u_recover; a.temperature = s.temperature;
    a.accept = s.accept; a.recovered = s.recovered;
    a.ws = static_cast<char*>(s.workspace);
    a.x_rs = s.logits_row_stride; a.q_rs = s.probs_row_stride; a.par_bs = s.parents_batch_stride;
    a.ws_per_row = spec_ws_per_row(s.vocab);
    a.T = s.nodes; a.V = s.vocab; a.C = (int)spec_accept_chunks(s.vocab);
    a.temperature_value = s.temperature_value;
    const int64_t rows = s.batch * s.nodes;
    if (s.dtype == FA_BF16) launch_spec_accept_t<bf16_tag>(a, rows, s.probs_dtype, stream);
    else if (s.dtype == FA_FP16) launch_spec_accept_t<fp16_tag>(a, rows, s.probs_dtype, stream);
    else launch_spec_accept_t<fp32_tag>(a, rows, s.probs_dtype, stream);
}

void launch_spec_walk(const fa_spec_walk_params& s, hipStream_t stream) {
    spec::SpWalkArgs a;
    a.parents = s.parents; a.draft_ids = s.draft_ids; a.target_ids = s.target_ids;
    a.accept = s.accept; a.recovered = s.recovered;
    a.out_tokens = s.out_tokens; a.num_out = s.num_out; a.path_nodes = s.path_nodes;
    a.par_bs = s.parents_batch_stride; a.tid_bs = s.target_ids_batch_stride; a.tid_ns = s.target_ids_node_stride;
    a.T = s.nodes;
    hipLaunchKernelGGL(spec::spec_walk_kernel, dim3((unsigned)s.batch), dim3(64), 0, stream, a);
}

}  // namespace fa
