// fa_sample.hip - token sampling from [rows, vocab] logits (fa_sample, include/fa_mi355.h): temperature, top-k, min-p, top-p and
// one inverse-CDF draw from a caller-supplied uniform number per row; fp16 / bf16 / fp32 logits.  The rules are in the header; in
// short, the row's statistics, its e_j and its integer masses q_j = floor(e_j * 2^40) are fa_mass.h's - the arithmetic this op shares
// with fa_spec_accept (fa_spec_verify.hip), the row view, the statistics sweep, the draw target and the walk step included -
// and every decision after that is INTEGER arithmetic on the q_j - a sum of them does not depend on the order of addition, so the
// LDS integer adds below cost no repeatability.  No float atomics, no host synchronisation, no RNG: capturable.
// Launch plan below SM_SPLIT_MIN columns: ONE workgroup of 1024 lanes per row, no workspace (the split plan for longer rows is
// described in front of its kernels, further down: the same sweeps, a launch each).  A piece is 8 columns counted from column 0 of the row; wave w owns
// the contiguous run of ITERS x 64 pieces behind wave w - 1's (ITERS = ceil(ceil(vocab / 8) / 1024): a function of vocab alone), lane
// l of it the pieces l, l + 64, .. of that run.  A piece is one 16-byte load (fp32: two) where the row starts on a 16-byte boundary
// and the piece lies inside the row, element by element otherwise: the same values, never a column >= vocab.
// A row runs these sweeps over its logits, each with a trip count of ITERS (a sweep that a row does not need is left out as a whole):
//     stats            fa_lse.h's (m, s) over x, the first maximum j*, n0 = the number of values above -inf
//     masses           (min_p, or top_p without top_k) sum q, and the count / mass / lowest key of the values with e_j >= min_p
//     select x BITS/8  (top_k by count, top_p by mass) a radix select over the order-preserving integer key of v_j, 8 bits a sweep
//                      (16-bit logits: 2, fp32: 4): a 256-bin histogram of counts (u32) and masses (u64) in LDS, 8 copies of each bin
//                      (lane & 7) and a run of equal bins merged in the lane before it is added;  the cut is (K, c): every key above
//                      K and the first c (in index order) of the keys equal to K
//     ties             (only where c is not the whole class) the index of the c-th key equal to K: per-wave counts, then the one
//                      wave that holds it walks its run again
//     draw             per-wave kept mass -> Q, rr = min(floor(u Q), Q - 1), then the one wave that holds rr walks its run again
//     filtered         the logit's own bits where kept, -inf elsewhere
// Every walk is an in-wave shuffle scan; no loop depends on the data.
#include "fa_mass.h"

namespace fa {

constexpr int SM_REP = 8;                                 // copies of every histogram bin
constexpr int SM_ALL = MASS_NONE;                         // tie index: the whole class is kept

// the order-preserving integer key of a canonical value (no NaN, no -0): a larger value has a larger key, equal values equal keys
__device__ __forceinline__ uint32_t sm_key32(float v) {
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
template <typename T> struct SmKey;
template <> struct SmKey<fp32_tag> {
    static constexpr int BITS = 32;
    static __device__ __forceinline__ uint32_t key(float v) { return sm_key32(v); }
};
template <> struct SmKey<bf16_tag> {
    static constexpr int BITS = 16;
    static __device__ __forceinline__ uint32_t key(float v) { return sm_key32(v) >> 16; }
};
template <> struct SmKey<fp16_tag> {
    static constexpr int BITS = 16;
    static __device__ __forceinline__ uint32_t key(float v) {
        const uint32_t h = __builtin_bit_cast(uint16_t, (_Float16)v);           // (exact: v came from an fp16)
        return h ^ ((h & 0x8000u) ? 0xffffu : 0x8000u);
    }
};

struct SmShared {
    uint64_t mass[256 * SM_REP];
    uint64_t tmass[256];
    uint64_t slot64[2 * MASS_WAVES];
    uint64_t cum_m, sel_mass;
    uint32_t cnt[256 * SM_REP];
    uint32_t tcnt[256];
    uint32_t slot32[2 * MASS_WAVES];
    float slotf[3 * MASS_WAVES];
    uint32_t sel_bin, cum_c, sel_cnt;
    int found;
};

struct SmArgs {
    const void* x;
    const float* u;
    const float* temperature;
    const int32_t* top_k;
    const float* top_p;
    const float* min_p;
    int32_t* ids;
    int32_t* n_kept;
    float* lse;
    void* filtered;
    int64_t x_rs, f_rs;
    int V, iters;
    float temperature_value, top_p_value, min_p_value;
    int32_t top_k_value;
};

// the kept set: every key above K and the keys equal to K at an index <= I
struct SmCut { uint32_t K; int I; };
__device__ __forceinline__ bool sm_kept(const SmCut& c, uint32_t key, int idx) { return key > c.K || (key == c.K && idx <= c.I); }

// block sums / minimum: EVERY lane of the workgroup calls them (they hold barriers)
__device__ __forceinline__ uint64_t sm_block_sum64(uint64_t v, SmShared& sh, int wave, int lane) {
    for (int m = 1; m < 64; m <<= 1) v += shfl_xor64(v, m);
    if (lane == 0) sh.slot64[wave] = v;
    __syncthreads();
    uint64_t t = 0;
    for (int w = 0; w < MASS_WAVES; ++w) t += sh.slot64[w];
    __syncthreads();
    return t;
}
__device__ __forceinline__ uint32_t sm_block_sum32(uint32_t v, SmShared& sh, int wave, int lane) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    if (lane == 0) sh.slot32[wave] = v;
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < MASS_WAVES; ++w) t += sh.slot32[w];
    __syncthreads();
    return t;
}
__device__ __forceinline__ uint32_t sm_block_min32(uint32_t v, SmShared& sh, int wave, int lane) {
    for (int m = 1; m < 64; m <<= 1) { const uint32_t o = __shfl_xor(v, m); v = o < v ? o : v; }
    if (lane == 0) sh.slot32[wave] = v;
    __syncthreads();
    uint32_t t = 0xffffffffu;
    for (int w = 0; w < MASS_WAVES; ++w) t = sh.slot32[w] < t ? sh.slot32[w] : t;
    __syncthreads();
    return t;
}

// wave 0: the bin, from 255 downwards, in which the running count (mass) reaches `target` >= 1
template <bool BY_MASS>
__device__ __forceinline__ void sm_find_bin(SmShared& sh, uint64_t target, int lane) {
    uint32_t cc[4];
    uint64_t mc[4];
    uint32_t sc = 0;
    uint64_t sm = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = 255 - 4 * lane - j;
        cc[j] = sh.tcnt[b];
        mc[j] = sh.tmass[b];
        sc += cc[j];
        sm += mc[j];
    }
    uint32_t ic = sc;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(ic, off);
        if (lane >= off) ic += t;
    }
    uint32_t run_c = ic - sc;
    uint64_t run_m = wave_scan64(sm, lane) - sm;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t cum = BY_MASS ? run_m : (uint64_t)run_c;
        const uint64_t w = BY_MASS ? mc[j] : (uint64_t)cc[j];
        if (cum < target && target <= cum + w) {
            sh.sel_bin = (uint32_t)(255 - 4 * lane - j);
            sh.cum_c = run_c;
            sh.cum_m = run_m;
            sh.sel_cnt = cc[j];
            sh.sel_mass = mc[j];
        }
        run_c += cc[j];
        run_m += mc[j];
    }
}

struct SmSel { uint32_t K, above_c, cls; uint64_t above_m, qK, rest; };   // rest: what of the target the class K has to give

// the radix select over the keys of the values above -inf: the key K at which the running count (BY_MASS: mass), taken in
// descending key order, reaches `target`
template <typename T, bool BY_MASS>
__device__ __forceinline__ SmSel sm_select(const MassRow<T>& r, SmShared& sh, float inv_t, float m, uint64_t target) {
    constexpr int BITS = SmKey<T>::BITS;
    const uint32_t kneg = SmKey<T>::key(-INFINITY);
    const int tid = r.wave * 64 + r.lane;
    SmSel s = {0, 0, 0, 0, 0, 0};
    uint64_t cls_mass = 0;
    for (int d = 0; d < BITS / 8; ++d) {
        const int shift = BITS - 8 * (d + 1);
        for (int j = tid; j < 256 * SM_REP; j += MASS_THREADS) { sh.cnt[j] = 0; sh.mass[j] = 0; }
        if (tid == 0) { sh.sel_bin = 0; sh.cum_c = 0; sh.cum_m = 0; sh.sel_cnt = 0; sh.sel_mass = 0; }
        __syncthreads();
        int cur = -1;
        uint32_t cur_c = 0;
        uint64_t cur_m = 0;
        const int rep = r.lane & (SM_REP - 1);
        for (int i = 0; i < r.iters; ++i) {
            const int c = r.col(i);
            if (c >= r.V) continue;
            float v[8];
            r.values(c, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t key = SmKey<T>::key(v[e]);
                const bool part = key != kneg && (uint32_t)((uint64_t)key >> (shift + 8)) == s.K;
                if (part) {
                    const int bin = (int)((key >> shift) & 255u);
                    if (bin != cur) {
                        if (cur_c) {
                            atomicAdd(&sh.cnt[cur * SM_REP + rep], cur_c);
                            if (cur_m) atomicAdd((unsigned long long*)&sh.mass[cur * SM_REP + rep], (unsigned long long)cur_m);
                        }
                        cur = bin; cur_c = 0; cur_m = 0;
                    }
                    cur_c += 1;
                    cur_m += mass_q(mass_e(v[e], inv_t, m));
                }
            }
        }
        if (cur_c) {
            atomicAdd(&sh.cnt[cur * SM_REP + rep], cur_c);
            if (cur_m) atomicAdd((unsigned long long*)&sh.mass[cur * SM_REP + rep], (unsigned long long)cur_m);
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t tc = 0;
            uint64_t tm = 0;
#pragma unroll
            for (int j = 0; j < SM_REP; ++j) { tc += sh.cnt[tid * SM_REP + j]; tm += sh.mass[tid * SM_REP + j]; }
            sh.tcnt[tid] = tc;
            sh.tmass[tid] = tm;
        }
        __syncthreads();
        if (r.wave == 0) sm_find_bin<BY_MASS>(sh, target, r.lane);
        __syncthreads();
        s.K = (s.K << 8) | sh.sel_bin;
        s.above_c += sh.cum_c;
        s.above_m += sh.cum_m;
        target -= BY_MASS ? sh.cum_m : (uint64_t)sh.cum_c;
        s.cls = sh.sel_cnt;
        cls_mass = sh.sel_mass;
        __syncthreads();                                         // (every wave has read the slots before the next reset)
    }
    s.qK = s.cls ? cls_mass / s.cls : 0;                         // (the class has one value: its masses are equal)
    s.rest = target;
    return s;
}

// the per-wave sums of a weight over the row (sh.slot64[wave]); returns their total.  EVERY lane calls it
template <typename T, typename W>
__device__ __forceinline__ uint64_t sm_wave_totals(const MassRow<T>& r, SmShared& sh, const W& weight) {
    uint64_t s = 0;
    for (int i = 0; i < r.iters; ++i) {
        const int c = r.col(i);
        if (c >= r.V) continue;
        float v[8];
        r.values(c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += weight(v[e], c + e);
    }
    for (int m = 1; m < 64; m <<= 1) s += shfl_xor64(s, m);
    if (r.lane == 0) sh.slot64[MASS_WAVES + r.wave] = s;
    __syncthreads();
    uint64_t t = 0;
    for (int w = 0; w < MASS_WAVES; ++w) t += sh.slot64[MASS_WAVES + w];
    return t;
}

// behind sm_wave_totals of the same weight: the smallest index whose index-order running weight exceeds `at`; `fallback` where
// the total does not.  EVERY lane calls it
template <typename T, typename W>
__device__ __forceinline__ int sm_find_index(const MassRow<T>& r, SmShared& sh, const W& weight, uint64_t at, int fallback) {
    uint64_t base = 0;
    int wstar = -1;
    for (int w = 0; w < MASS_WAVES; ++w) {
        const uint64_t t = sh.slot64[MASS_WAVES + w];
        if (wstar < 0) {
            if (base + t > at) wstar = w;
            else base += t;
        }
    }
    if (r.wave == 0 && r.lane == 0) sh.found = fallback;
    __syncthreads();
    if (r.wave == wstar) {
        uint64_t running = base;
        for (int i = 0; i < r.iters; ++i) {
            const int c = r.col(i);
            uint64_t wv[8];
            uint64_t ls = 0;
            if (c < r.V) {
                float v[8];
                r.values(c, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) { wv[e] = weight(v[e], c + e); ls += wv[e]; }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) wv[e] = 0;
            }
            mass_walk_step(wv, ls, running, at, c, r.lane, sh.found);
        }
    }
    __syncthreads();
    return sh.found;
}

template <typename T>
__global__ void __launch_bounds__(MASS_THREADS) sample_kernel(const SmArgs a) {
    __shared__ SmShared sh;
    const int64_t row = blockIdx.x;
    const MassRow<T> r = mass_row_whole<T>(a.x, row * a.x_rs, a.V, a.iters);
    const bool lane0 = threadIdx.x == 0;

    // ---- stats: (m, s) over x, the first maximum, n0 - in every lane
    const float temp = a.temperature ? a.temperature[row] : a.temperature_value;
    const MassStat stat = mass_stats(r, mass_inv_t(temp), sh.slotf, sh.slot32, true);
    __syncthreads();                                              // (the slots are used again below)
    const MassNode n = mass_node(stat, temp);
    const float inv_t = n.inv_t, m = n.m;

    const uint32_t kneg = SmKey<T>::key(-INFINITY);
    int id = -1;
    uint32_t n_kept = 0;
    SmCut cut = {SmKey<T>::key(INFINITY), -1};                    // nothing
    if (lane0 && a.lse) a.lse[row] = n.empty ? -INFINITY : n.st.m + logf(n.st.s);

    if (!n.empty && n.greedy) {
        id = n.bi;
        n_kept = 1;
        cut = SmCut{SmKey<T>::key(n.bv), n.bi};
    } else if (!n.empty) {
        const int32_t k = a.top_k ? a.top_k[row] : a.top_k_value;
        const float top_p = a.top_p ? a.top_p[row] : a.top_p_value;
        const float min_p = a.min_p ? a.min_p[row] : a.min_p_value;
        const bool k_on = k >= 1 && (uint32_t)k < n.n0;
        const bool p_on = top_p < 1.0f;
        const bool mp_on = min_p > 0.f;
        const float mp = fminf(min_p, 1.0f);

        uint32_t K = kneg, c = 0, cls = 0, above_c = n.n0;        // the cut (K, c): every value above -inf
        uint64_t mass = 0;                                        // the kept mass, where a later step needs it
        if (k_on) {
            const SmSel s = sm_select<T, false>(r, sh, inv_t, m, (uint64_t)k);
            K = s.K; c = (uint32_t)s.rest; cls = s.cls; above_c = s.above_c;
            mass = s.above_m + (uint64_t)c * s.qK;
        }
        if (mp_on || (p_on && !k_on)) {
            uint64_t qtot = 0, m_mp = 0;
            uint32_t n_mp = 0, k_mp = 0xffffffffu;
            for (int i = 0; i < r.iters; ++i) {
                const int cc = r.col(i);
                if (cc >= r.V) continue;
                float v[8];
                r.values(cc, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float ee = mass_e(v[e], inv_t, m);
                    const uint64_t q = mass_q(ee);
                    qtot += q;
                    if (v[e] > -INFINITY && ee >= mp) {
                        const uint32_t key = SmKey<T>::key(v[e]);
                        n_mp += 1;
                        m_mp += q;
                        k_mp = key < k_mp ? key : k_mp;
                    }
                }
            }
            qtot = sm_block_sum64(qtot, sh, r.wave, r.lane);
            if (!k_on) mass = qtot;
            if (mp_on) {
                m_mp = sm_block_sum64(m_mp, sh, r.wave, r.lane);
                n_mp = sm_block_sum32(n_mp, sh, r.wave, r.lane);
                k_mp = sm_block_min32(k_mp, sh, r.wave, r.lane);
                if (n_mp < above_c + c) {                         // the values with e_j >= mp: whole classes, down to key k_mp
                    K = k_mp - 1; c = 0; cls = 0; above_c = n_mp; mass = m_mp;
                }
            }
        }
        if (p_on) {
            const double t = ceil((double)top_p * (double)mass);
            const uint64_t tq = t >= 1.0 ? (uint64_t)t : 1ull;
            const SmSel s = sm_select<T, true>(r, sh, inv_t, m, tq);
            uint64_t need = s.qK ? (s.rest + s.qK - 1) / s.qK : 1;
            if (need > s.cls) need = s.cls;
            K = s.K; c = (uint32_t)need; cls = s.cls; above_c = s.above_c;
        }
        n_kept = above_c + c;
        cut.K = K;
        if (c == 0) {
            cut.I = -1;
        } else if (c >= cls) {
            cut.I = SM_ALL;
        } else {
            auto tie = [K](float v, int) -> uint64_t { return SmKey<T>::key(v) == K ? 1ull : 0ull; };
            sm_wave_totals(r, sh, tie);
            cut.I = sm_find_index(r, sh, tie, (uint64_t)c - 1, SM_ALL);
        }
        if (a.ids) {
            const SmCut kc = cut;
            auto kept_q = [kc, inv_t, m](float v, int idx) -> uint64_t {
                return sm_kept(kc, SmKey<T>::key(v), idx) ? mass_q(mass_e(v, inv_t, m)) : 0ull;
            };
            const uint64_t Q = sm_wave_totals(r, sh, kept_q);
            id = sm_find_index(r, sh, kept_q, mass_draw_target(a.u[row], Q), n.bi);
        }
    }
    if (lane0) {
        if (a.ids) a.ids[row] = id;
        if (a.n_kept) a.n_kept[row] = (int32_t)n_kept;
    }
    if (!a.filtered) return;
    // ---- filtered: the logit's own bits where kept
    const int64_t foff = row * a.f_rs;
    const bool vec_out = mass_row_vec<T>(a.filtered, foff);
    for (int i = 0; i < r.iters; ++i) {
        const int c = r.col(i);
        if (c >= r.V) continue;
        float v[8];
        r.raw(c, -INFINITY, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = sm_kept(cut, SmKey<T>::key(mass_canon(v[e])), c + e) ? v[e] : -INFINITY;
        if (vec_out && c + 8 <= r.V) {
            RowIo<T>::store8(a.filtered, foff + c, v);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c + e < r.V) RowIo<T>::store1(a.filtered, foff + c + e, v[e]);
        }
    }
}

// ================================================================================================================================
// The split plan (vocab >= SM_SPLIT_MIN): a row is cut into C = ceil(vocab / MASS_CHUNK) chunks, one workgroup of 1024 lanes each
// (2 pieces per lane; wave w of chunk c owns run c * 16 + w of the row, so the index order of the runs is the one-workgroup plan's),
// and every step of the one-workgroup kernel that meets over the whole row becomes a launch of its own on the stream:
//     stats    rows x C   chunk (m, s), first maximum, n0                    -> ws: one 32-byte partial per chunk (plain stores)
//     resolve  rows       merges them in chunk order, reads the row's parameters, writes lse, settles empty / greedy rows and
//                         writes the row's RECORD: what the next sweep is (a select digit, the masses, the tie or draw totals)
//     phase    rows x C   the record's sweep over the chunk: an LDS histogram added to the row's 256 bins in the workspace with
//                         integer atomics / the masses' sums with integer atomics / one total per run (plain stores)
//     resolve  rows       takes that result (finds the bin; applies min_p; walks the one run that holds the tie or the draw),
//                         zeroes what it has read and advances the record
//     ..       phase + resolve as often as the longest row can need: a function of the dtype and of which filters CAN be on
//     filtered rows x C   the kept set of the record
// No workgroup waits for another; the workspace needs no initialisation (the first resolve zeroes the bins before any add).
// Integer adds commute, the float partials are merged in chunk order: a row's bits depend on (vocab, dtype) and its values alone.
constexpr int SM_SPLIT_MIN = 2 * MASS_CHUNK;
enum { SM_DONE = 0, SM_SELK = 1, SM_MASS = 2, SM_SELP = 3, SM_TIE = 4, SM_DRAW = 5 };

struct SmRec {
    float m, inv_t, bv, mp, top_p;
    int bi, next, digit, I;
    uint32_t n0, K, c, cls, above_c, k_on, p_on, mp_on;
    uint32_t sel_prefix, sel_above_c;
    uint64_t mass, sel_above_m, sel_target;
};
struct SmMassAcc { unsigned long long qtot, m_mp; uint32_t n_mp, kmp_inv, pad[2]; };
static_assert(sizeof(SmRec) <= 256 && sizeof(SmMassAcc) == 32, "the workspace layout");

// a row's part of the workspace
struct SmWs {
    char* base;
    int C;
    int64_t per_row;
    __device__ __forceinline__ char* row(int64_t r) const { return base + r * per_row; }
    __device__ __forceinline__ SmRec* rec(int64_t r) const { return reinterpret_cast<SmRec*>(row(r)); }
    __device__ __forceinline__ SmMassAcc* acc(int64_t r) const { return reinterpret_cast<SmMassAcc*>(row(r) + 256); }
    __device__ __forceinline__ uint32_t* cnt(int64_t r) const { return reinterpret_cast<uint32_t*>(row(r) + 320); }
    __device__ __forceinline__ unsigned long long* mass(int64_t r) const { return reinterpret_cast<unsigned long long*>(row(r) + 1344); }
    __device__ __forceinline__ MassStat* stat(int64_t r) const { return reinterpret_cast<MassStat*>(row(r) + 3392); }
    __device__ __forceinline__ uint64_t* tot(int64_t r) const { return reinterpret_cast<uint64_t*>(row(r) + 3392 + 32 * C); }
};
inline int sample_chunks(int V) { return (V + MASS_CHUNK - 1) / MASS_CHUNK; }
inline int64_t sample_ws_per_row(int V) {
    const int64_t C = sample_chunks(V);
    return (3392 + 32 * C + 8 * MASS_WAVES * C + 255) / 256 * 256;
}

template <typename T>
__device__ __forceinline__ MassRow<T> sm_chunk_row(const SmArgs& a, int64_t row, int chunk) {
    return mass_row_chunk<T>(a.x, row * a.x_rs, a.V, chunk);
}

// f(column, canonical values) for the lane's pieces that have a column < V, in index order
template <typename T, typename F>
__device__ __forceinline__ void sm_pieces(const MassRow<T>& r, F&& f) {
    for (int i = 0; i < r.iters; ++i) {
        const int c = r.col(i);
        if (c >= r.V) continue;
        float v[8];
        r.values(c, v);
        f(c, v);
    }
}

// the weight of the tie walk (the keys equal to K) and of the draw walk (the kept masses) of a record
template <typename T>
__device__ __forceinline__ uint64_t sm_rec_weight(const SmRec& rc, float v, int idx) {
    const uint32_t key = SmKey<T>::key(v);
    if (rc.next == SM_TIE) return key == rc.K ? 1ull : 0ull;
    return sm_kept(SmCut{rc.K, rc.I}, key, idx) ? mass_q(mass_e(v, rc.inv_t, rc.m)) : 0ull;
}

template <typename T>
__global__ void __launch_bounds__(MASS_THREADS) sample_stats_kernel(const SmArgs a, const SmWs ws) {
    __shared__ SmShared sh;
    const int64_t row = (int64_t)blockIdx.x / ws.C;
    const int chunk = (int)((int64_t)blockIdx.x - row * ws.C);
    const MassRow<T> r = sm_chunk_row<T>(a, row, chunk);
    const float temp = a.temperature ? a.temperature[row] : a.temperature_value;
    const MassStat o = mass_stats(r, mass_inv_t(temp), sh.slotf, sh.slot32, threadIdx.x == 0);
    if (threadIdx.x == 0) ws.stat(row)[chunk] = o;
}

template <typename T>
__global__ void __launch_bounds__(MASS_THREADS) sample_phase_kernel(const SmArgs a, const SmWs ws) {
    __shared__ SmShared sh;
    const int64_t row = (int64_t)blockIdx.x / ws.C;
    const int chunk = (int)((int64_t)blockIdx.x - row * ws.C);
    const SmRec rc = *ws.rec(row);
    if (rc.next == SM_DONE) return;
    const MassRow<T> r = sm_chunk_row<T>(a, row, chunk);
    const int tid = (int)threadIdx.x;
    if (rc.next == SM_SELK || rc.next == SM_SELP) {
        constexpr int BITS = SmKey<T>::BITS;
        const uint32_t kneg = SmKey<T>::key(-INFINITY);
        const int shift = BITS - 8 * (rc.digit + 1);
        for (int j = tid; j < 256 * SM_REP; j += MASS_THREADS) { sh.cnt[j] = 0; sh.mass[j] = 0; }
        __syncthreads();
        int cur = -1;
        uint32_t cur_c = 0;
        uint64_t cur_m = 0;
        const int rep = r.lane & (SM_REP - 1);
        sm_pieces(r, [&](int, const float (&v)[8]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t key = SmKey<T>::key(v[e]);
                const bool part = key != kneg && (uint32_t)((uint64_t)key >> (shift + 8)) == rc.sel_prefix;
                if (part) {
                    const int bin = (int)((key >> shift) & 255u);
                    if (bin != cur) {
                        if (cur_c) {
                            atomicAdd(&sh.cnt[cur * SM_REP + rep], cur_c);
                            if (cur_m) atomicAdd((unsigned long long*)&sh.mass[cur * SM_REP + rep], (unsigned long long)cur_m);
                        }
                        cur = bin; cur_c = 0; cur_m = 0;
                    }
                    cur_c += 1;
                    cur_m += mass_q(mass_e(v[e], rc.inv_t, rc.m));
                }
            }
        });
        if (cur_c) {
            atomicAdd(&sh.cnt[cur * SM_REP + rep], cur_c);
            if (cur_m) atomicAdd((unsigned long long*)&sh.mass[cur * SM_REP + rep], (unsigned long long)cur_m);
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t tc = 0;
            unsigned long long tm = 0;
#pragma unroll
            for (int j = 0; j < SM_REP; ++j) { tc += sh.cnt[tid * SM_REP + j]; tm += sh.mass[tid * SM_REP + j]; }
            if (tc) atomicAdd(&ws.cnt(row)[tid], tc);
            if (tm) atomicAdd(&ws.mass(row)[tid], tm);
        }
    } else if (rc.next == SM_MASS) {
        uint64_t qtot = 0, m_mp = 0;
        uint32_t n_mp = 0, k_mp = 0xffffffffu;
        sm_pieces(r, [&](int, const float (&v)[8]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ee = mass_e(v[e], rc.inv_t, rc.m);
                const uint64_t q = mass_q(ee);
                qtot += q;
                if (v[e] > -INFINITY && ee >= rc.mp) {
                    const uint32_t key = SmKey<T>::key(v[e]);
                    n_mp += 1;
                    m_mp += q;
                    k_mp = key < k_mp ? key : k_mp;
                }
            }
        });
        qtot = sm_block_sum64(qtot, sh, r.wave, r.lane);
        m_mp = sm_block_sum64(m_mp, sh, r.wave, r.lane);
        n_mp = sm_block_sum32(n_mp, sh, r.wave, r.lane);
        k_mp = sm_block_min32(k_mp, sh, r.wave, r.lane);
        if (tid == 0) {
            SmMassAcc* acc = ws.acc(row);
            if (qtot) atomicAdd(&acc->qtot, (unsigned long long)qtot);
            if (m_mp) atomicAdd(&acc->m_mp, (unsigned long long)m_mp);
            if (n_mp) atomicAdd(&acc->n_mp, n_mp);
            atomicMax(&acc->kmp_inv, ~k_mp);
        }
    } else {                                              // SM_TIE / SM_DRAW: one total per run
        uint64_t s = 0;
        sm_pieces(r, [&](int c, const float (&v)[8]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) s += sm_rec_weight<T>(rc, v[e], c + e);
        });
        for (int m = 1; m < 64; m <<= 1) s += shfl_xor64(s, m);
        if (r.lane == 0) ws.tot(row)[r.run] = s;
    }
}

// what follows the filters of a record: n_kept, and the tie walk where the cut class is kept in part
__device__ __forceinline__ void sm_after_filters(SmRec& rc, bool want_ids) {
    if (rc.c == 0) rc.I = -1;
    else if (rc.c >= rc.cls) rc.I = SM_ALL;
    else { rc.next = SM_TIE; return; }
    rc.next = want_ids ? SM_DRAW : SM_DONE;
}
__device__ __forceinline__ void sm_start_select(SmRec& rc, int kind, uint64_t target) {
    rc.next = kind; rc.digit = 0; rc.sel_prefix = 0; rc.sel_above_c = 0; rc.sel_above_m = 0; rc.sel_target = target;
}
__device__ __forceinline__ void sm_start_top_p(SmRec& rc) {
    const double t = ceil((double)rc.top_p * (double)rc.mass);
    sm_start_select(rc, SM_SELP, t >= 1.0 ? (uint64_t)t : 1ull);
}

template <typename T>
__global__ void __launch_bounds__(MASS_THREADS) sample_resolve_kernel(const SmArgs a, const SmWs ws, const int first) {
    __shared__ SmShared sh;
    const int64_t row = blockIdx.x;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t kneg = SmKey<T>::key(-INFINITY);
    constexpr int ND = SmKey<T>::BITS / 8;
    const bool want_ids = a.ids != nullptr;
    SmRec rc;
    if (first) {
        const MassStat stat = mass_merge(ws.stat(row), ws.C);
        const MassNode n = mass_node(stat, a.temperature ? a.temperature[row] : a.temperature_value);
        if (tid == 0 && a.lse) a.lse[row] = n.empty ? -INFINITY : n.st.m + logf(n.st.s);
        if (tid < 256) { ws.cnt(row)[tid] = 0; ws.mass(row)[tid] = 0; }
        if (tid == 0) { SmMassAcc z = {0, 0, 0, 0, {0, 0}}; *ws.acc(row) = z; }
        rc = SmRec{};
        rc.m = n.m; rc.inv_t = n.inv_t; rc.bv = n.bv; rc.bi = n.bi; rc.n0 = n.n0;
        if (n.empty || n.greedy) {
            rc.next = SM_DONE;
            rc.K = n.empty ? SmKey<T>::key(INFINITY) : SmKey<T>::key(n.bv);
            rc.I = n.empty ? -1 : n.bi;
            if (tid == 0) {
                if (a.ids) a.ids[row] = n.empty ? -1 : n.bi;
                if (a.n_kept) a.n_kept[row] = n.empty ? 0 : 1;
                *ws.rec(row) = rc;
            }
            return;
        }
        const int32_t k = a.top_k ? a.top_k[row] : a.top_k_value;
        const float min_p = a.min_p ? a.min_p[row] : a.min_p_value;
        rc.top_p = a.top_p ? a.top_p[row] : a.top_p_value;
        rc.k_on = k >= 1 && (uint32_t)k < n.n0;
        rc.p_on = rc.top_p < 1.0f;
        rc.mp_on = min_p > 0.f;
        rc.mp = fminf(min_p, 1.0f);
        rc.K = kneg; rc.c = 0; rc.cls = 0; rc.above_c = n.n0; rc.mass = 0;
        if (rc.k_on) sm_start_select(rc, SM_SELK, (uint64_t)k);
        else if (rc.mp_on || rc.p_on) rc.next = SM_MASS;
        else sm_after_filters(rc, want_ids);
    } else {
        rc = *ws.rec(row);
        if (rc.next == SM_DONE) return;
        if (rc.next == SM_SELK || rc.next == SM_SELP) {
            const bool by_mass = rc.next == SM_SELP;
            if (tid < 256) {
                sh.tcnt[tid] = ws.cnt(row)[tid];
                sh.tmass[tid] = ws.mass(row)[tid];
                ws.cnt(row)[tid] = 0;
                ws.mass(row)[tid] = 0;
            }
            if (tid == 0) { sh.sel_bin = 0; sh.cum_c = 0; sh.cum_m = 0; sh.sel_cnt = 0; sh.sel_mass = 0; }
            __syncthreads();
            if (wave == 0) {
                if (by_mass) sm_find_bin<true>(sh, rc.sel_target, lane);
                else sm_find_bin<false>(sh, rc.sel_target, lane);
            }
            __syncthreads();
            rc.sel_prefix = (rc.sel_prefix << 8) | sh.sel_bin;
            rc.sel_above_c += sh.cum_c;
            rc.sel_above_m += sh.cum_m;
            rc.sel_target -= by_mass ? sh.cum_m : (uint64_t)sh.cum_c;
            rc.digit += 1;
            if (rc.digit == ND) {
                const uint32_t cls = sh.sel_cnt;
                const uint64_t qK = cls ? sh.sel_mass / cls : 0;
                rc.K = rc.sel_prefix; rc.cls = cls; rc.above_c = rc.sel_above_c;
                if (!by_mass) {
                    rc.c = (uint32_t)rc.sel_target;
                    rc.mass = rc.sel_above_m + (uint64_t)rc.c * qK;
                    if (rc.mp_on) rc.next = SM_MASS;
                    else if (rc.p_on) sm_start_top_p(rc);
                    else sm_after_filters(rc, want_ids);
                } else {
                    uint64_t need = qK ? (rc.sel_target + qK - 1) / qK : 1;
                    if (need > cls) need = cls;
                    rc.c = (uint32_t)need;
                    sm_after_filters(rc, want_ids);
                }
            }
        } else if (rc.next == SM_MASS) {
            const SmMassAcc acc = *ws.acc(row);
            __syncthreads();
            if (tid == 0) { SmMassAcc z = {0, 0, 0, 0, {0, 0}}; *ws.acc(row) = z; }
            if (!rc.k_on) rc.mass = acc.qtot;
            if (rc.mp_on && acc.n_mp < rc.above_c + rc.c) {
                rc.K = ~acc.kmp_inv - 1; rc.c = 0; rc.cls = 0; rc.above_c = acc.n_mp; rc.mass = acc.m_mp;
            }
            if (rc.p_on) sm_start_top_p(rc);
            else sm_after_filters(rc, want_ids);
        } else {                                          // SM_TIE / SM_DRAW: the run that holds the target, then its walk
            const int U = ws.C * MASS_WAVES;
            for (int j = tid; j < U; j += MASS_THREADS) sh.mass[j] = ws.tot(row)[j];
            if (tid == 0) sh.found = rc.next == SM_TIE ? SM_ALL : rc.bi;
            __syncthreads();
            uint64_t at;
            if (rc.next == SM_TIE) {
                at = (uint64_t)rc.c - 1;
            } else {
                uint64_t Q = 0;
                for (int j = 0; j < U; ++j) Q += sh.mass[j];
                at = mass_draw_target(a.u[row], Q);
            }
            uint64_t base = 0;
            int ustar = -1;
            for (int j = 0; j < U; ++j) {
                const uint64_t t = sh.mass[j];
                if (ustar < 0) {
                    if (base + t > at) ustar = j;
                    else base += t;
                }
            }
            if (wave == 0 && ustar >= 0) {
                MassRow<T> r = sm_chunk_row<T>(a, row, 0);
                r.run = ustar;
                uint64_t running = base;
                for (int i = 0; i < r.iters; ++i) {
                    const int c = r.col(i);
                    uint64_t wv[8];
                    uint64_t ls = 0;
                    if (c < r.V) {
                        float v[8];
                        r.values(c, v);
#pragma unroll
                        for (int e = 0; e < 8; ++e) { wv[e] = sm_rec_weight<T>(rc, v[e], c + e); ls += wv[e]; }
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) wv[e] = 0;
                    }
                    mass_walk_step(wv, ls, running, at, c, lane, sh.found);
                }
            }
            __syncthreads();
            if (rc.next == SM_TIE) {
                rc.I = sh.found;
                rc.next = want_ids ? SM_DRAW : SM_DONE;
            } else {
                if (tid == 0) a.ids[row] = sh.found;
                rc.next = SM_DONE;
            }
        }
    }
    // (every path to here has passed a barrier or read the record before any lane can reach this store)
    __syncthreads();
    if (tid == 0) {
        if ((rc.next == SM_TIE || rc.next == SM_DRAW || rc.next == SM_DONE) && a.n_kept) a.n_kept[row] = (int32_t)(rc.above_c + rc.c);
        *ws.rec(row) = rc;
    }
}

template <typename T>
__global__ void __launch_bounds__(MASS_THREADS) sample_filtered_kernel(const SmArgs a, const SmWs ws) {
    const int64_t row = (int64_t)blockIdx.x / ws.C;
    const int chunk = (int)((int64_t)blockIdx.x - row * ws.C);
    const SmRec rc = *ws.rec(row);
    const SmCut cut = {rc.K, rc.I};
    const MassRow<T> r = sm_chunk_row<T>(a, row, chunk);
    const int64_t foff = row * a.f_rs;
    const bool vec_out = mass_row_vec<T>(a.filtered, foff);
    for (int i = 0; i < r.iters; ++i) {
        const int c = r.col(i);
        if (c >= r.V) continue;
        float v[8];
        r.raw(c, -INFINITY, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = sm_kept(cut, SmKey<T>::key(mass_canon(v[e])), c + e) ? v[e] : -INFINITY;
        if (vec_out && c + 8 <= r.V) {
            RowIo<T>::store8(a.filtered, foff + c, v);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c + e < r.V) RowIo<T>::store1(a.filtered, foff + c + e, v[e]);
        }
    }
}

// ---- the host side: the launch plan is a function of vocab (and, for the number of launches, of the dtype and of which filters
// can be on) alone
int sample_iters(int V) {
    const int64_t pieces = ((int64_t)V + 7) / 8;
    return (int)((pieces + MASS_THREADS - 1) / MASS_THREADS);
}
int64_t sample_chunks_per_row(int V) { return V >= SM_SPLIT_MIN ? sample_chunks(V) : 1; }
size_t sample_workspace_bytes(int64_t rows, int V, int) {
    return V >= SM_SPLIT_MIN && rows > 0 ? (size_t)rows * (size_t)sample_ws_per_row(V) : 0;
}

template <typename T>
static void launch_sample_split(const fa_sample_params& s, const SmArgs& a, hipStream_t stream) {
    SmWs ws;
    ws.base = static_cast<char*>(s.workspace);
    ws.C = sample_chunks(s.vocab);
    ws.per_row = sample_ws_per_row(s.vocab);
    const dim3 gc((unsigned)(s.rows * ws.C)), gr((unsigned)s.rows), b(MASS_THREADS);
    // the sweeps the longest row can need
    const bool sampled = s.temperature || s.temperature_value > 0.f;
    const bool k_can = s.top_k || s.top_k_value >= 1;
    const bool p_can = s.top_p || s.top_p_value < 1.0f;
    const bool mp_can = s.min_p || s.min_p_value > 0.f;
    const int nd = SmKey<T>::BITS / 8;
    const int phases = !sampled ? 0 : nd * (int)k_can + (int)(mp_can || p_can) + nd * (int)p_can + 1 + (s.ids ? 1 : 0);
    hipLaunchKernelGGL((sample_stats_kernel<T>), gc, b, 0, stream, a, ws);
    hipLaunchKernelGGL((sample_resolve_kernel<T>), gr, b, 0, stream, a, ws, 1);
    for (int p = 0; p < phases; ++p) {
        hipLaunchKernelGGL((sample_phase_kernel<T>), gc, b, 0, stream, a, ws);
        hipLaunchKernelGGL((sample_resolve_kernel<T>), gr, b, 0, stream, a, ws, 0);
    }
    if (s.filtered) hipLaunchKernelGGL((sample_filtered_kernel<T>), gc, b, 0, stream, a, ws);
}

// The caller (fa_api.hip) has validated the block; rows > 0
void launch_sample(const fa_sample_params& s, hipStream_t stream) {
    SmArgs a;
    a.x = s.logits; a.u = s.u;
    a.temperature = s.temperature; a.top_k = s.top_k; a.top_p = s.top_p; a.min_p = s.min_p;
    a.ids = s.ids; a.n_kept = s.n_kept; a.lse = s.lse; a.filtered = s.filtered;
    a.x_rs = s.logits_row_stride; a.f_rs = s.filtered_row_stride;
    a.V = s.vocab; a.iters = sample_iters(s.vocab);
    a.temperature_value = s.temperature_value; a.top_p_value = s.top_p_value; a.min_p_value = s.min_p_value;
    a.top_k_value = s.top_k_value;
    if (s.vocab >= SM_SPLIT_MIN) {
        if (s.dtype == FA_BF16) launch_sample_split<bf16_tag>(s, a, stream);
        else if (s.dtype == FA_FP16) launch_sample_split<fp16_tag>(s, a, stream);
        else launch_sample_split<fp32_tag>(s, a, stream);
        return;
    }
    const dim3 g((unsigned)s.rows), b(MASS_THREADS);
    if (s.dtype == FA_BF16) hipLaunchKernelGGL((sample_kernel<bf16_tag>), g, b, 0, stream, a);
    else if (s.dtype == FA_FP16) hipLaunchKernelGGL((sample_kernel<fp16_tag>), g, b, 0, stream, a);
    else hipLaunchKernelGGL((sample_kernel<fp32_tag>), g, b, 0, stream, a);
}

}  // namespace fa
