// fa_spec_verify.hip - speculative-decoding verification (fa_spec_accept, fa_spec_walk; include/fa_mi355.h): the rejection-sampling
// decision of every draft node from its target row of logits and its draft row of probabilities, and the one-wave walk that turns
// the decisions into emitted tokens and the accepted path.  The rules are in the header; in short, per node with target row
// values v_j (a NaN counts as -inf, -0 as +0), d the draft token and q_j the draft probabilities as they are:
//     x_j = v_j * inv_t,  m = x_{j*},  e_j = e(x_j - m)  (fa_sample's masses),  s = fa_lse.h's sum-exp,  p_j = e_j * (1.0f / s)
//     accept = (uu * q_d < p_d);   r_j = min(max(p_j - q_j, 0), 1),  R_j = floor(r_j * 2^40)  (uint64),  R = sum R_j
//     R == 0: R_j := floor(e_j * 2^40);   recovered = the smallest index whose running sum of R_j exceeds min(floor(uu_r R), R - 1)
// Everything behind the R_j is INTEGER arithmetic: the sums do not depend on the order of addition.  No float atomics, no RNG, no
// host synchronisation: capturable.
// Launch plan, a function of vocab alone: a row is cut into C = ceil(vocab / SP_CHUNK) chunks, one workgroup of 1024 lanes each (2
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
#include <cmath>
#include <cstdint>
#include "fa_lse.h"

namespace fa {
namespace spec {

constexpr int SP_THREADS = 1024;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_CHUNK = 16384;                           // columns per workgroup
constexpr int SP_ITERS = SP_CHUNK / 8 / SP_THREADS;       // pieces per lane
constexpr int SP_NONE = 0x7fffffff;

struct f32_tag {};

// one element / one whole piece of a row's type (fa_sample.hip's SmIo, loads only)
template <typename T> struct SpIo {
    static constexpr int ESIZE = 2;
    static __device__ __forceinline__ float load1(const void* p, int64_t at) {
        return Elem<T>::lo((uint32_t) static_cast<const uint16_t*>(p)[at]);
    }
    static __device__ __forceinline__ void load8(const void* p, int64_t at, float (&v)[8]) { row_load8<T>(p, at, false, v); }
};
template <> struct SpIo<f32_tag> {
    static constexpr int ESIZE = 4;
    static __device__ __forceinline__ float load1(const void* p, int64_t at) { return static_cast<const float*>(p)[at]; }
    static __device__ __forceinline__ void load8(const void* p, int64_t at, float (&v)[8]) { row_load8<bf16_tag>(p, at, true, v); }
};

__device__ __forceinline__ float sp_canon(float v) { return v != v ? -INFINITY : (v == 0.f ? 0.f : v); }

// e_j, its integer mass, and the residual of (p_j, q_j) - restated from fa_sample.hip (sm_e, sm_q): the same bits
__device__ __forceinline__ float sp_e(float v, float inv_t, float m) { return lse_exp(v * inv_t - m); }
__device__ __forceinline__ uint64_t sp_q(float e) { return e > 0.f ? (uint64_t)(e * 1099511627776.0f) : 0ull; }
__device__ __forceinline__ float sp_r(float p, float q) {
    float r = p - q;
    r = r > 0.f ? r : 0.f;                                // (a NaN difference: 0)
    return r < 1.f ? r : 1.f;
}

__device__ __forceinline__ uint64_t sp_shfl_up64(uint64_t v, int off) {
    const uint32_t lo = __shfl_up((uint32_t)v, off), hi = __shfl_up((uint32_t)(v >> 32), off);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t sp_shfl_xor64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t sp_shfl64(uint64_t v, int lane) {
    const uint32_t lo = __shfl((uint32_t)v, lane), hi = __shfl((uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}
// the inclusive sum over the lanes 0 .. own of the wave
__device__ __forceinline__ uint64_t sp_wave_scan64(uint64_t v, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t t = sp_shfl_up64(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

struct SpStat { float m, s, bv; int bi; uint32_t n0, pad[3]; };
struct SpSums { unsigned long long R, E; };
static_assert(sizeof(SpStat) == 32 && sizeof(SpSums) == 16, "the workspace layout");

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
    __device__ __forceinline__ SpStat* stat(int64_t row) const { return reinterpret_cast<SpStat*>(ws + row * ws_per_row); }
    __device__ __forceinline__ SpSums* sums(int64_t row) const { return reinterpret_cast<SpSums*>(ws + row * ws_per_row + 32 * C); }
};

// node `row` = (b, t): its parent, or -1 for node 0 and for a padding node
__device__ __forceinline__ int sp_parent(const SpArgs& a, int64_t row, int64_t& b) {
    b = row / a.T;
    const int t = (int)(row - b * a.T);
    if (t == 0) return -1;
    const int par = a.parents ? a.parents[b * a.par_bs + t] : t - 1;
    return par >= 0 && par < t ? par : -1;
}

// a row as a lane sees it
template <typename T> struct SpRow {
    const void* p;
    int64_t rowoff;
    int V, wave, lane;
    bool vec;
    __device__ __forceinline__ SpRow(const void* base, int64_t off, int vocab) {
        p = base; rowoff = off; V = vocab;
        wave = (int)threadIdx.x >> 6;
        lane = (int)threadIdx.x & 63;
        vec = ((reinterpret_cast<uintptr_t>(base) + (uint64_t)off * SpIo<T>::ESIZE) & 15) == 0;
    }
    __device__ __forceinline__ int col(int chunk, int i) const { return 8 * (((chunk * SP_WAVES + wave) * SP_ITERS + i) * 64 + lane); }
    // the raw values of the piece at column c (c < V); columns >= V: fill
    __device__ __forceinline__ void raw(int c, float fill, float (&r)[8]) const {
        if (vec && c + 8 <= V) {
            SpIo<T>::load8(p, rowoff + c, r);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = c + i < V ? SpIo<T>::load1(p, rowoff + c + i) : fill;
        }
    }
    // the canonical logits
    __device__ __forceinline__ void values(int c, float (&v)[8]) const {
        raw(c, -INFINITY, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = sp_canon(v[i]);
    }
};

__device__ __forceinline__ float sp_inv_t(const SpArgs& a, int64_t b, bool& cold) {
    const float temp = a.temperature ? a.temperature[b] : a.temperature_value;
    cold = !(temp > 0.f);
    return cold ? 1.0f : 1.0f / temp;
}

template <typename T>
__global__ void __launch_bounds__(SP_THREADS) spec_stats_kernel(const SpArgs a) {
    __shared__ float slotf[3 * SP_WAVES];
    __shared__ uint32_t slot32[2 * SP_WAVES];
    const int64_t row = (int64_t)blockIdx.x / a.C;
    const int chunk = (int)((int64_t)blockIdx.x - row * a.C);
    int64_t b;
    const int par = sp_parent(a, row, b);
    if (par < 0) return;
    bool cold;
    const float inv_t = sp_inv_t(a, b, cold);
    const SpRow<T> r(a.x, (b * a.T + par) * a.x_rs, a.V);
    LseState st = {-INFINITY, 0.f};
    float bv = -INFINITY;
    int bi = SP_NONE;
    uint32_t n0 = 0;
    for (int i = 0; i < SP_ITERS; ++i) {
        const int c = r.col(chunk, i);
        if (c >= r.V) continue;
        float v[8], x[8];
        r.values(c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[e] = v[e] * inv_t;
            if (v[e] > bv) { bv = v[e]; bi = c + e; }
            n0 += v[e] > -INFINITY ? 1u : 0u;
        }
        lse_piece(st, x);
    }
    st = lse_wave(st);
    for (int m = 1; m < 64; m <<= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        n0 += __shfl_xor(n0, m);
    }
    if (r.lane == 0) {
        slotf[r.wave] = st.m;
        slotf[SP_WAVES + r.wave] = st.s;
        slotf[2 * SP_WAVES + r.wave] = bv;
        slot32[r.wave] = (uint32_t)bi;
        slot32[SP_WAVES + r.wave] = n0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    st = LseState{slotf[0], slotf[SP_WAVES]};
    bv = slotf[2 * SP_WAVES];
    bi = (int)slot32[0];
    n0 = slot32[SP_WAVES];
    for (int w = 1; w < SP_WAVES; ++w) {
        st = lse_merge(st, LseState{slotf[w], slotf[SP_WAVES + w]});
        const float ov = slotf[2 * SP_WAVES + w];
        const int oi = (int)slot32[w];
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        n0 += slot32[SP_WAVES + w];
    }
    const SpStat o = {st.m, st.s, bv, bi, n0, {0, 0, 0}};
    a.stat(row)[chunk] = o;
}

// what a node's partials say, merged in chunk order: the same bits in every workgroup that asks
struct SpNode { float m, s, inv_t; int bi; bool empty, greedy; };
__device__ __forceinline__ SpNode sp_node(const SpArgs& a, int64_t row, int64_t b) {
    const SpStat* sp = a.stat(row);
    SpStat o = sp[0];
    LseState st = {o.m, o.s};
    float bv = o.bv;
    int bi = o.bi;
    uint32_t n0 = o.n0;
    for (int c = 1; c < a.C; ++c) {
        o = sp[c];
        st = lse_merge(st, LseState{o.m, o.s});
        if (o.bv > bv || (o.bv == bv && o.bi < bi)) { bv = o.bv; bi = o.bi; }
        n0 += o.n0;
    }
    SpNode n;
    bool cold;
    n.inv_t = sp_inv_t(a, b, cold);
    n.m = bv * n.inv_t;                                   // x_{j*}: the maximum of the running pair (the product is monotone)
    n.s = st.s;
    n.bi = bi;
    n.empty = n0 == 0;
    n.greedy = cold || !(fabsf(n.m) < INFINITY);          // (+inf in the row, or 1 / T overflows the product)
    return n;
}

template <typename T, typename Q>
__global__ void __launch_bounds__(SP_THREADS) spec_mass_kernel(const SpArgs a) {
    __shared__ uint64_t slot64[2 * SP_WAVES];
    const int64_t row = (int64_t)blockIdx.x / a.C;
    const int chunk = (int)((int64_t)blockIdx.x - row * a.C);
    int64_t b;
    const int par = sp_parent(a, row, b);
    if (par < 0) return;
    const SpNode n = sp_node(a, row, b);
    if (n.empty || n.greedy) return;
    const float inv_s = 1.0f / n.s;
    const SpRow<T> xr(a.x, (b * a.T + par) * a.x_rs, a.V);
    const SpRow<Q> qr(a.q, row * a.q_rs, a.V);
    uint64_t R = 0, E = 0;
    for (int i = 0; i < SP_ITERS; ++i) {
        const int c = xr.col(chunk, i);
        if (c >= a.V) continue;
        float v[8], q[8];
        xr.values(c, v);
        qr.raw(c, 0.f, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float ee = sp_e(v[e], n.inv_t, n.m);
            E += sp_q(ee);
            R += sp_q(sp_r(ee * inv_s, q[e]));
        }
    }
    for (int m = 1; m < 64; m <<= 1) { R += sp_shfl_xor64(R, m); E += sp_shfl_xor64(E, m); }
    if (xr.lane == 0) { slot64[xr.wave] = R; slot64[SP_WAVES + xr.wave] = E; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    SpSums o = {0, 0};
    for (int w = 0; w < SP_WAVES; ++w) { o.R += slot64[w]; o.E += slot64[SP_WAVES + w]; }
    a.sums(row)[chunk] = o;
}

template <typename T, typename Q>
__global__ void __launch_bounds__(SP_THREADS) spec_final_kernel(const SpArgs a) {
    __shared__ uint64_t wtot[SP_WAVES];
    __shared__ int found;
    const int64_t row = blockIdx.x;
    const bool lane0 = threadIdx.x == 0;
    int64_t b;
    const int par = sp_parent(a, row, b);
    if (par < 0) {
        if (lane0) { a.accept[row] = 0; a.recovered[row] = -1; }
        return;
    }
    const SpNode n = sp_node(a, row, b);
    const int d = a.draft_ids[row];
    if (n.empty || n.greedy) {
        if (lane0) {
            a.accept[row] = !n.empty && d == n.bi ? 1 : 0;
            a.recovered[row] = n.empty ? -1 : n.bi;
        }
        return;
    }
    const float inv_s = 1.0f / n.s;
    const SpRow<T> xr(a.x, (b * a.T + par) * a.x_rs, a.V);
    const SpRow<Q> qr(a.q, row * a.q_rs, a.V);
    // ---- the totals; R == 0: the target's own masses
    const SpSums* sums = a.sums(row);
    uint64_t R = 0, E = 0;
    for (int c = 0; c < a.C; ++c) { R += sums[c].R; E += sums[c].E; }
    const bool own = R == 0;
    const uint64_t tot = own ? E : R;                     // (> 0: e_{j*} = 1)
    const float ur = a.u_recover[row];
    const double uu_r = ur > 0.f ? (double)ur : 0.0;
    const double fl = floor(uu_r * (double)tot);
    uint64_t rr = fl >= 18446744073709551615.0 ? tot : (uint64_t)fl;
    if (rr > tot - 1) rr = tot - 1;
    uint64_t base = 0;
    int cstar = -1;
    for (int c = 0; c < a.C; ++c) {
        const uint64_t t = own ? sums[c].E : sums[c].R;
        if (cstar < 0) {
            if (base + t > rr) cstar = c;
            else base += t;
        }
    }
    // ---- accept
    if (lane0) {
        bool acc = false;
        if (d >= 0 && d < a.V) {
            const float pd = sp_e(sp_canon(SpIo<T>::load1(a.x, xr.rowoff + d)), n.inv_t, n.m) * inv_s;
            const float qd = SpIo<Q>::load1(a.q, qr.rowoff + d);
            const float ua = a.u_accept[row];
            const float uu = ua > 0.f ? ua : 0.f;
            acc = uu * qd < pd;
        }
        a.accept[row] = acc ? 1 : 0;
        found = n.bi;
    }
    // ---- the sweep of chunk cstar
    uint64_t wv[SP_ITERS][8];
    uint64_t ls[SP_ITERS];
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < SP_ITERS; ++i) {
        const int c = xr.col(cstar < 0 ? 0 : cstar, i);
        ls[i] = 0;
        if (cstar >= 0 && c < a.V) {
            float v[8], q[8];
            xr.values(c, v);
            if (!own) qr.raw(c, 0.f, q);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ee = sp_e(v[e], n.inv_t, n.m);
                wv[i][e] = own ? sp_q(ee) : sp_q(sp_r(ee * inv_s, q[e]));
                ls[i] += wv[i][e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) wv[i][e] = 0;
        }
        s += ls[i];
    }
    for (int m = 1; m < 64; m <<= 1) s += sp_shfl_xor64(s, m);
    if (xr.lane == 0) wtot[xr.wave] = s;
    __syncthreads();
    int wstar = -1;
    for (int w = 0; w < SP_WAVES; ++w) {
        const uint64_t t = wtot[w];
        if (wstar < 0) {
            if (base + t > rr) wstar = w;
            else base += t;
        }
    }
    if (xr.wave == wstar) {
        uint64_t running = base;
#pragma unroll
        for (int i = 0; i < SP_ITERS; ++i) {
            const int c = xr.col(cstar, i);
            const uint64_t incl = sp_wave_scan64(ls[i], xr.lane);
            uint64_t p = running + (incl - ls[i]);
            if (p <= rr && rr < p + ls[i]) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (p <= rr && rr < p + wv[i][e]) found = c + e;
                    p += wv[i][e];
                }
            }
            running += sp_shfl64(incl, 63);
        }
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
int64_t spec_accept_chunks(int V) { return ((int64_t)V + spec::SP_CHUNK - 1) / spec::SP_CHUNK; }
static int64_t spec_ws_per_row(int V) { return (48 * spec_accept_chunks(V) + 63) / 64 * 64; }
size_t spec_accept_workspace_bytes(int64_t rows, int V) { return rows > 0 ? (size_t)rows * (size_t)spec_ws_per_row(V) : 0; }

template <typename T, typename Q>
static void launch_spec_accept_tq(const spec::SpArgs& a, int64_t rows, hipStream_t stream) {
    const dim3 gc((unsigned)(rows * a.C)), gr((unsigned)rows), b(spec::SP_THREADS);
    hipLaunchKernelGGL((spec::spec_stats_kernel<T>), gc, b, 0, stream, a);
    hipLaunchKernelGGL((spec::spec_mass_kernel<T, Q>), gc, b, 0, stream, a);
    hipLaunchKernelGGL((spec::spec_final_kernel<T, Q>), gr, b, 0, stream, a);
}
template <typename T>
static void launch_spec_accept_t(const spec::SpArgs& a, int64_t rows, int probs_dtype, hipStream_t stream) {
    if (probs_dtype == FA_BF16) launch_spec_accept_tq<T, bf16_tag>(a, rows, stream);
    else if (probs_dtype == FA_FP16) launch_spec_accept_tq<T, fp16_tag>(a, rows, stream);
    else launch_spec_accept_tq<T, spec::f32_tag>(a, rows, stream);
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
    else launch_spec_accept_t<spec::f32_tag>(a, rows, s.probs_dtype, stream);
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
