// Seeded temperature / top-k / top-p sampling of the next token from a row of f32 logits, closing
// the decode loop on the device like the argmax path: one key (f32_ordered(l_tok) << 32) | ~tok per
// row, which decode_update consumes unchanged (nparts = 1).
//
// Definition (normative; models/gpt2.py reference_sample is the same in numpy):
//   l_j   = seen(j) ? (z_j < 0 ? z_j * penalty : z_j / penalty) : z_j               (f32)
//   key_j = (f32_ordered(l_j) << 32) | ~j, a total order; candidates = the k' = min(top_k, vocab)
//           largest keys, descending; columns >= vocab are never candidates
//   w_i   = exp((double)(l_i - l_0) / T), c_i = w_0 + ... + w_i in candidate order, W = c_{k'-1}
//   m     = top_p >= 1 ? k' : the smallest count with c_{m-1} >= top_p * W
//   u     = (Philox4x32-10(counter = (position, stream_lo, stream_hi, 0), key = seed)[0] >> 8) * 2^-24
//   token = the first i < m with c_i > u * c_{m-1}
//
// One 1024-thread workgroup per row.  The row is read from memory ONCE, into registers (float4
// chunk t + 1024 j of thread t: 13 chunks for GPT-2's 50304 padded columns); everything after that
// works on registers and a few KiB of LDS:
//   1. a lower bound on the k'-th largest key from group maxima: the threads form G >= k' disjoint
//      groups (waves, 16-lane rows or quads); each group's maximum is a distinct element, so the
//      smallest of the G maxima has at least G >= k' keys at or above it.  Elements below it
//      ("non-survivors", all but a few hundred of a typical row) take no part in the selection:
//      the survivors are listed in LDS (up to 2048; a row with more keeps selecting from the
//      registers, slower and with the same result).
//   2. an exact radix select of the k'-th largest 64-bit key among the survivors: six 8-bit digits
//      (four of the ordered value, two of ~index, whose upper 16 bits are all ones below 65536
//      columns), one 256-bin LDS histogram each.  The key order has no ties, so rows of equal
//      values select exactly k' elements like any other row, in a fixed number of passes.
//   3. the k' keys at or above the selected one are compacted into LDS, ranked against each other
//      (they are distinct), and the weights, prefix sums, nucleus and draw follow in double.
#include "common.h"

#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / 64)
#define SMP_MAX_K 256
#define SMP_SURV 2048  // survivor keys listed in LDS; rows with more select from the registers

__device__ __forceinline__ void philox4x32_10(unsigned int (&c)[4], unsigned int k0, unsigned int k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c[1] ^ k0;
        const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (unsigned int)p1;
        c[3] = (unsigned int)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// Philox known-answer hook for the tests: out[0..4) = Philox4x32-10(in[0..4), key in[4..6))
__global__ void philox_kernel(const unsigned int* __restrict__ in, unsigned int* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned int c[4] = {in[6 * i], in[6 * i + 1], in[6 * i + 2], in[6 * i + 3]};
    philox4x32_10(c, in[6 * i + 4], in[6 * i + 5]);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = c[j];
}

template <int NJ>
__global__ __launch_bounds__(SMP_THREADS) void sample_topk_topp_kernel(
    const float* __restrict__ logits, long long ldz, const unsigned int* __restrict__ seen, int seen_words,
    const int* __restrict__ lens, const long long* __restrict__ streams, const int* __restrict__ slot_map,
    int n_slots, const unsigned long long* __restrict__ seed_p, float penalty, double temperature, int top_k,
    double top_p, int vocab, unsigned long long* keys_out, long long ldk) {
    __shared__ __attribute__((aligned(16))) unsigned int hist[256];
    __shared__ unsigned long long cand[SMP_MAX_K];
    __shared__ unsigned long long sorted[SMP_MAX_K];
    __shared__ double wsum[SMP_MAX_K];  // weights, then their prefix sums in place
    __shared__ unsigned long long wave_min[SMP_WAVES];
    __shared__ unsigned long long surv[SMP_SURV];
    __shared__ unsigned int sel_digit, sel_rank, n_cand, n_surv, nucleus;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row = blockIdx.x;
    const int nv4 = (int)(ldz >> 2);
    const int kk0 = top_k < vocab ? top_k : vocab;  // k'

    // the row's state, requested with the logits (every lane reads the same words)
    const int b = slot_map ? (int)dlms_idx(slot_map[row], n_slots, CHK_SAMPLE_SLOT) : row;
    const int position = lens[b];
    const unsigned long long stream = (unsigned long long)streams[b];
    const unsigned long long seed = *seed_p;

    // ---- the row into registers: unconditional loads at clamped indices, values masked by the
    // column index afterwards (a load under a per-lane condition is emitted as branch, load, wait)
    const float4* zrow = reinterpret_cast<const float4*>(logits + (size_t)row * ldz);
    const unsigned int* srow = seen + (size_t)row * seen_words;
    float4 z[NJ];
    unsigned int sw[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = t + SMP_THREADS * j;
        const int ic = i < nv4 ? i : nv4 - 1;
        z[j] = zrow[ic];
        const int w = ic >> 3;  // 4 columns of a chunk share one 32-column bitmap word
        sw[j] = srow[w < seen_words ? w : seen_words - 1];
    }
    // penalised logits as ordered words (the float is recovered from a key where it is needed).
    // Element (j, e) is column 4 t + 4096 j + e: it exists iff 4096 j + e < vrem, and the low word of
    // its key is ~column = nbase - (4096 j + e) -- a compare and a subtract against constants, so the
    // passes below keep one register per element and nothing else across them
    const int vrem = vocab - 4 * t;
    const unsigned int nbase = ~(unsigned int)(4 * t);
    unsigned int ord[NJ][4];
    unsigned long long tmax = 0ull;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float v4[4] = {z[j].x, z[j].y, z[j].z, z[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int off = 4 * SMP_THREADS * j + e;
            float v = v4[e];
            if ((sw[j] >> ((4 * t + off) & 31)) & 1u) v = v < 0.f ? v * penalty : v / penalty;
            ord[j][e] = f32_ordered(v);
            const unsigned long long key = ((unsigned long long)ord[j][e] << 32) | (nbase - (unsigned int)off);
            if (off < vrem && key > tmax) tmax = key;
        }
    }

    // ---- 1. lower bound: the smallest of G >= k' group maxima (a group without a valid column
    // gives 0: no bound, everything survives)
    unsigned long long gmax;
    if (kk0 <= SMP_WAVES) {
        gmax = wave_max_u64(tmax);
    } else if (kk0 <= SMP_THREADS / 16) {
        gmax = row16_max_u64(tmax);
    } else {  // quads: 256 groups
        unsigned long long o = dpp_perm_u64<0xB1>(tmax);
        gmax = o > tmax ? o : tmax;
        o = dpp_perm_u64<0x4E>(gmax);
        gmax = o > gmax ? o : gmax;
    }
    const unsigned long long wmin = ~wave_max_u64(~gmax);
    if (lane == 0) wave_min[wave] = wmin;
    if (t < 256) hist[t] = 0u;
    if (t < SMP_MAX_K) {
        cand[t] = 0ull;
        sorted[t] = 0ull;
    }
    if (t == 0) {
        n_cand = 0u;
        n_surv = 0u;
    }
    __syncthreads();
    unsigned long long thr = wave_min[0];
#pragma unroll
    for (int w = 1; w < SMP_WAVES; ++w) thr = wave_min[w] < thr ? wave_min[w] : thr;

    // the survivors (a few hundred of a typical row) listed in LDS: the passes below then touch
    // only them.  A row with more survivors than the list holds selects from the registers instead
    // (all_listed is false for the whole workgroup) -- slower, the same result
    {
        const unsigned int thr_hi = (unsigned int)(thr >> 32);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int off = 4 * SMP_THREADS * j + e;
                if (off < vrem && ord[j][e] >= thr_hi) {
                    const unsigned long long key = ((unsigned long long)ord[j][e] << 32) | (nbase - (unsigned int)off);
                    if (key >= thr) {
                        const unsigned int p = atomicAdd(&n_surv, 1u);
                        if (p < SMP_SURV) surv[p] = key;
                    }
                }
            }
    }
    __syncthreads();
    const unsigned int ns = n_surv;
    const bool all_listed = ns <= SMP_SURV;

    // ---- 2. radix select of the k'-th largest key among the survivors (key >= thr).  The wanted
    // key lies in [lo, hi]: all keys of that range share the digits chosen so far
    unsigned long long lo = thr, hi = ~0ull;
    unsigned int rank = (unsigned int)kk0;  // the wanted key is the rank-th largest of the range
#pragma unroll 1
    for (int pass = 0; pass < 6; ++pass) {
        const int shift = pass < 4 ? 56 - 8 * pass : 8 - 8 * (pass - 4);
        if (all_listed) {
            for (unsigned int i = t; i < ns; i += SMP_THREADS) {
                const unsigned long long key = surv[i];
                if (key >= lo && key <= hi) atomicAdd(&hist[(unsigned int)(key >> shift) & 255u], 1u);
            }
        } else {
            const unsigned int lo_hi = (unsigned int)(lo >> 32), hi_hi = (unsigned int)(hi >> 32);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int off = 4 * SMP_THREADS * j + e;
                    if (off < vrem && ord[j][e] >= lo_hi && ord[j][e] <= hi_hi) {
                        const unsigned long long key =
                            ((unsigned long long)ord[j][e] << 32) | (nbase - (unsigned int)off);
                        if (key >= lo && key <= hi) atomicAdd(&hist[(unsigned int)(key >> shift) & 255u], 1u);
                    }
                }
        }
        __syncthreads();
        if (wave == 0) {
            // above(d) = keys of the range with a digit >= d; the wanted digit has above(d) >= rank >
            // above(d + 1).  Lane l owns digits 4 l .. 4 l + 3: a suffix sum over the lanes, then its four
            const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];
            const unsigned int own4 = (h.x + h.y) + (h.z + h.w);
            unsigned int suf = own4;  // -> sum over lanes >= this one
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned int o = __shfl_down(suf, off, 64);
                if (lane + off < 64) suf += o;
            }
            unsigned int above = suf - own4;  // digits of the lanes above
            const unsigned int own[4] = {h.w, h.z, h.y, h.x};
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // digits 4 l + 3 down to 4 l
                above += own[u];
                if (above >= rank && above - own[u] < rank) {
                    sel_digit = (unsigned int)(4 * lane + 3 - u);
                    sel_rank = rank - (above - own[u]);
                }
            }
        }
        __syncthreads();
        // digits above this one are equal in lo's range and hi (pass 0: none are fixed yet)
        const unsigned long long fixed = (pass == 0 ? 0ull : hi & (~0ull << (shift + 8))) |
                                         ((unsigned long long)sel_digit << shift);
        unsigned long long nlo = fixed;
        hi = fixed | ((1ull << shift) - 1ull);
        if (pass == 3) nlo |= 0xffff0000ull;  // ~column of a column below 65536: no digits to choose there
        lo = nlo > lo ? nlo : lo;
        rank = sel_rank;
        // (the histogram was last read before the barrier above; the selection words are next
        // written behind the next pass's first barrier)
        if (t < 256) hist[t] = 0u;
        __syncthreads();
    }
    // lo == hi is now the k'-th largest key: exactly k' keys are >= it

    // ---- 3. compact, rank, weigh
    if (all_listed) {
        for (unsigned int i = t; i < ns; i += SMP_THREADS) {
            const unsigned long long key = surv[i];
            if (key >= lo) {
                const unsigned int p = atomicAdd(&n_cand, 1u);
                if (p < SMP_MAX_K) cand[p] = key;
            }
        }
    } else {
        const unsigned int lo_hi = (unsigned int)(lo >> 32);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int off = 4 * SMP_THREADS * j + e;
                if (off < vrem && ord[j][e] >= lo_hi) {
                    const unsigned long long key = ((unsigned long long)ord[j][e] << 32) | (nbase - (unsigned int)off);
                    if (key >= lo) {
                        const unsigned int p = atomicAdd(&n_cand, 1u);
                        if (p < SMP_MAX_K) cand[p] = key;
                    }
                }
            }
    }
    __syncthreads();
    const int kc = kk0 < SMP_MAX_K ? kk0 : SMP_MAX_K;
    if (t < kc) {
        const unsigned long long mine = cand[t];
        int r = 0;
        for (int u = 0; u < kc; ++u) r += cand[u] > mine ? 1 : 0;  // (same address in every lane: a broadcast)
        sorted[r] = mine;
    }
    __syncthreads();
    if (t < kc) {
        const float l0 = f32_from_ordered((unsigned int)(sorted[0] >> 32));
        const float li = f32_from_ordered((unsigned int)(sorted[t] >> 32));
        wsum[t] = exp((double)(li - l0) / temperature);
    }
    __syncthreads();
    if (t == 0) {  // prefix sums in candidate order (the definition's order: a serial chain of <= 256 adds)
        double c = 0.0;
        for (int i0 = 0; i0 < kc; i0 += 8) {  // eight loads in flight, then the eight adds in order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = wsum[i0 + u < kc ? i0 + u : kc - 1];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + u < kc) {
                    c += v[u];
                    wsum[i0 + u] = c;
                }
            }
        }
        nucleus = (unsigned int)kc;
    }
    __syncthreads();
    if (top_p < 1.0 && t < kc) {
        const double cut = top_p * wsum[kc - 1];
        if (wsum[t] >= cut && (t == 0 || !(wsum[t - 1] >= cut))) nucleus = (unsigned int)(t + 1);
    }
    __syncthreads();
    const int m = (int)nucleus;
    if (t < m) {
        unsigned int c[4] = {(unsigned int)position, (unsigned int)stream, (unsigned int)(stream >> 32), 0u};
        philox4x32_10(c, (unsigned int)seed, (unsigned int)(seed >> 32));
        const double u = (double)(c[0] >> 8) * (1.0 / 16777216.0);
        const double target = u * wsum[m - 1];
        if (wsum[t] > target && (t == 0 || !(wsum[t - 1] > target))) {
            const unsigned long long key = sorted[t];
            dlms_idx((long long)(unsigned int)~(unsigned int)key, vocab, CHK_SAMPLE_TOKEN);
            keys_out[(size_t)row * ldk] = key;
        }
    }
}

// logits [B][ldz] f32 (columns >= vocab ignored), seen [B][seen_words] (rows parallel to the logits
// rows), lens / streams indexed by the row's slot (row i, or slot_map[i]), one key per row out.
extern "C" hipError_t dlms_sample_topk_topp(const float* logits, long long ldz, const unsigned int* seen,
                                            int seen_words, const int* lens, const long long* streams, const int* slot_map,
                                            int n_slots, const unsigned long long* seed, float penalty,
                                            double temperature, int top_k, double top_p, int vocab,
                                            unsigned long long* keys_out, long long ldk, int B, hipStream_t stream) {
    if (B <= 0 || vocab < 1 || vocab > 65536 || ldz < vocab || ldz % 4 || ldz > 4ll * SMP_THREADS * 16 ||
        ((uintptr_t)logits & 15) || top_k < 1 || top_k > SMP_MAX_K || !(temperature > 0.0) ||
        !(top_p > 0.0 && top_p <= 1.0) || seen_words * 32ll < vocab || !(penalty > 0.f) || ldk < 1)
        return hipErrorInvalidValue;
    const int nv4 = (int)(ldz / 4);
#define SMP_LAUNCH(NJ)                                                                                          \
    hipLaunchKernelGGL(sample_topk_topp_kernel<NJ>, dim3(B), dim3(SMP_THREADS), 0, stream, logits, ldz, seen,  \
                       seen_words, lens, streams, slot_map, n_slots, seed, penalty, temperature, top_k, top_p, \
                       vocab, keys_out, ldk)
    if (nv4 <= SMP_THREADS * 1) SMP_LAUNCH(1);
    else if (nv4 <= SMP_THREADS * 4) SMP_LAUNCH(4);
    else if (nv4 <= SMP_THREADS * 13) SMP_LAUNCH(13);  // GPT-2: 50304 padded columns
    else SMP_LAUNCH(16);
#undef SMP_LAUNCH
    return hipGetLastError();
}

extern "C" hipError_t dlms_philox4x32_10(const unsigned int* in, unsigned int* out, int n, hipStream_t stream) {
    if (n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(philox_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, in, out, n);
    return hipGetLastError();
}

DLMS_CHECK_EXPORT(sample)
