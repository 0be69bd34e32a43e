// Token/position embedding (K1) and the per-step greedy bookkeeping that closes the decode loop
// on the device (K11/K12 consumer), so a whole decode step replays as one hipGraph with no host
// round trip: argmax key -> token -> output buffer, seen-bitmap, stop flags, next embedding.
#include "common.h"

// x[r] = wte[tokens[r]] + wpe[positions[r]]   (bf16 tables, f32 residual stream).  Wave per row.
__global__ __launch_bounds__(256) void embed_kernel(const int* __restrict__ tokens, const int* __restrict__ positions,
                                                    const bf16_t* __restrict__ wte, const bf16_t* __restrict__ wpe,
                                                    float* x, int ldx, int R, int D, int V, int P) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const bf16_t* a = wte + (size_t)dlms_idx(tokens[r], V, CHK_EMBED_TOKEN) * D;
    const bf16_t* b = wpe + (size_t)dlms_idx(positions[r], P, CHK_EMBED_POS) * D;
    float* o = x + (size_t)r * ldx;
    for (int c = lane; c < D / 8; c += 64) {
        float fa[8], fb[8];
        unpack8(*reinterpret_cast<const uint4*>(a + c * 8), fa);
        unpack8(*reinterpret_cast<const uint4*>(b + c * 8), fb);
        float4 lo = make_float4(fa[0] + fb[0], fa[1] + fb[1], fa[2] + fb[2], fa[3] + fb[3]);
        float4 hi = make_float4(fa[4] + fb[4], fa[5] + fb[5], fa[6] + fb[6], fa[7] + fb[7]);
        reinterpret_cast<float4*>(o + c * 8)[0] = lo;
        reinterpret_cast<float4*>(o + c * 8)[1] = hi;
    }
}

// max over a row's partial argmax keys, one wave per row (keys(b, p) = keys[b * sb + p * sp]), in
// rounds of 16 keys per lane.  The LM head leaves ~800 partial keys per row at TP=1: one round.
// A round's loads are unconditional -- the index is clamped to the last key and the value masked
// afterwards -- so all 16 issue back to back behind one wait.  (Guarded as `p < nparts ? keys[..] : 0`
// the compiler emits branch, load, full wait per key: a load is never hoisted out of a
// data-dependent condition.  The fix add_layernorm_kernel documents for itself.)
#define KEY_ROUND 16
__device__ __forceinline__ void key_round_load(const unsigned long long* __restrict__ keys, int b, int nparts,
                                               long long sb, long long sp, int lane, int p0,
                                               unsigned long long (&k)[KEY_ROUND]) {
#pragma unroll
    for (int u = 0; u < KEY_ROUND; ++u) {
        const int p = p0 + lane + 64 * u;
        k[u] = keys[(size_t)b * sb + (size_t)(p < nparts ? p : nparts - 1) * sp];
    }
}
__device__ __forceinline__ unsigned long long key_round_max(const unsigned long long (&k)[KEY_ROUND], int nparts,
                                                            int lane, int p0, unsigned long long best) {
#pragma unroll
    for (int u = 0; u < KEY_ROUND; ++u) {
        const unsigned long long v = p0 + lane + 64 * u < nparts ? k[u] : 0ull;
        best = v > best ? v : best;
    }
    return best;
}
// rounds from p0 on, folded into `best` (per lane; the caller reduces across the wave)
__device__ __forceinline__ unsigned long long key_rounds_from(const unsigned long long* __restrict__ keys, int b,
                                                              int nparts, long long sb, long long sp, int lane,
                                                              int p0, unsigned long long best) {
    for (; p0 < nparts; p0 += 64 * KEY_ROUND) {
        unsigned long long k[KEY_ROUND];
        key_round_load(keys, b, nparts, sb, sp, lane, p0, k);
        best = key_round_max(k, nparts, lane, p0, best);
    }
    return best;
}
__device__ __forceinline__ unsigned long long wave_key_max(const unsigned long long* __restrict__ keys, int b,
                                                           int nparts, long long sb, long long sp, int lane) {
    return wave_max_u64(key_rounds_from(keys, b, nparts, sb, sp, lane, 0, 0ull));  // identical in every lane
}

// argmax partials [B][nparts] -> one key per row (before the cross-rank all-gather under TP)
__global__ __launch_bounds__(256) void argmax_reduce_kernel(const unsigned long long* __restrict__ keys, int nparts,
                                                            long long sb, unsigned long long* out, int B) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const unsigned long long best = wave_key_max(keys, b, nparts, sb, 1, lane);
    if (lane == 0) out[b] = best;
}

#define DU_MAXV4 8  // float4 chunks of the new row per lane: D <= 64 * 8 * 4 = 2048

// One wave per live sequence b.
//   keys(b, p)   packed (ordered value, ~index) argmax keys: the LM head's per-column-tile
//                partials (TP=1) or the all-gathered per-rank keys (TP>1); max over p
//   lens[b]      tokens so far (prompt + generated);  finished[b] stop flag
//   out_tokens   [B][max_len] full sequences (prompt already written by the host)
//   seen         [B][seen_words] repetition-penalty bitmap
// Writes the next forward's token/position/kv-length for row b and its embedding into x.
// slot_map (optional): key row i updates sequence slot slot_map[i] -- used when a prefill of new
// requests lands in arbitrary free slots of a running continuous batch.
// Dependency chain: three memory round trips -- (1) the row's length and stop flag together with the
// first round of keys, (2) what the length addresses (positional-embedding row, a finished row's
// last token) together with the LayerNorm weights, (3) the token's embedding row.  Every load of a
// batch is unconditional (clamped index, value masked or unused afterwards): a load under a
// per-lane condition is emitted as branch, load, full wait, which made each batch a chain of its own.
//
// STOP (GenerationControls.stop; the definition is in controls.hip): after the token is written at
// index p the row also finishes when for a stop sequence s of length m both p + 1 - m >= P (the
// row's prompt length: the match lies wholly in generated tokens) and seq[p+1-m : p+1] == s.  The
// table holds STOP_MAX_SEQS sequences of up to STOP_MAX_LEN ids (length 0: unused).  Lane
// u < 32 owns element j = u & 7 of sequence u >> 3: the table and the prompt length load with round
// trip (1), the row's token at p + 1 - m + j (clamped; one of the last STOP_MAX_LEN - 1 tokens)
// with prev_tok in round trip (2), and a ballot whose byte is all ones is a hit.  Everything else
// is the code below, instruction for instruction: STOP = false is the kernel as it was.
#define STOP_MAX_SEQS 4
#define STOP_MAX_LEN 8
template <bool STOP>
struct StopArgs {};  // (an empty kernel argument: the launch of STOP = false passes what it always passed)
template <>
struct StopArgs<true> {
    const int* __restrict__ prompt_len;  // [slots]
    const int* __restrict__ stop_len;    // [STOP_MAX_SEQS]
    const int* __restrict__ stop_tok;    // [STOP_MAX_SEQS][STOP_MAX_LEN]
};
template <bool STOP>
__global__ __launch_bounds__(256) void decode_update_kernel(const unsigned long long* __restrict__ keys, int nparts,
                                                            long long sb, long long sp,
                                                            const int* __restrict__ slot_map, int* lens,
                                                            int* finished, int* out_tokens, int max_len,
                                                            unsigned int* seen, int seen_words, int* cur_tok,
                                                            int* cur_pos, int* cur_kvlen,
                                                            const bf16_t* __restrict__ wte,
                                                            const bf16_t* __restrict__ wpe, float* x, int ldx, int B,
                                                            int D, int eos, int t_max, int n_slots, int V,
                                                            const float* __restrict__ ln_g,
                                                            const float* __restrict__ ln_b, float eps, bf16_t* h,
                                                            int ldh, StopArgs<STOP> st) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    const int b = slot_map ? (int)dlms_idx(slot_map[i], n_slots, CHK_UPDATE_SLOT) : i;
    // row state (every lane reads the same words: one request each)
    const int len0 = (int)dlms_idx(lens[b], max_len + 1, CHK_UPDATE_LEN);
    const int fin = finished[b];
    unsigned long long k0[KEY_ROUND];  // in flight with lens / finished
    key_round_load(keys, i, nparts, sb, sp, lane, 0, k0);
    int st_m = 0, st_tok = 0, st_P = 0;
    if constexpr (STOP) {  // (indices masked to the table: lanes >= 32 repeat lanes < 32 and are not counted)
        st_m = st.stop_len[(lane >> 3) & (STOP_MAX_SEQS - 1)];
        st_tok = st.stop_tok[lane & (STOP_MAX_SEQS * STOP_MAX_LEN - 1)];
        st_P = st.prompt_len[b];
    }
    __builtin_amdgcn_sched_barrier(0);  // (the scheduler would otherwise move them behind the wait for len0)
    // where a live row's token goes (a finished row may sit at len == max_len: not an index then)
    const int live_len = fin ? 0 : (int)dlms_idx(len0, max_len, CHK_UPDATE_LEN);
    int pos = fin ? len0 - 1 : live_len;  // (length after this step) - 1
    pos = pos < 0 ? 0 : (pos < t_max - 1 ? pos : t_max - 1);
    // (a live row's len0 - 1 is a valid index too: read it anyway, use it only for a finished row)
    const int prev_tok = out_tokens[(size_t)b * max_len + (len0 > 0 ? len0 - 1 : 0)];
    const int last_tok = fin ? prev_tok : 0;
    int st_at = 0, st_have = 0;  // this lane's element of its stop sequence: index in the row, the token there
    if constexpr (STOP) {
        st_m = st_m < 0 ? 0 : (st_m > STOP_MAX_LEN ? STOP_MAX_LEN : st_m);
        st_at = live_len + 1 - st_m + (lane & (STOP_MAX_LEN - 1));
        const int at = st_at < 0 ? 0 : (st_at < max_len ? st_at : max_len - 1);
        st_have = out_tokens[(size_t)b * max_len + at];
    }
    // the row in float4 chunks c = lane + 64 j -- add_layernorm_kernel's partition, so the fused
    // LayerNorm below computes exactly what that kernel would on the stored row; chunks past the
    // row (c >= nv) read the row's last chunk and are never used
    const int nv = D >> 2;
    uint2 pe[DU_MAXV4];
#pragma unroll
    for (int j = 0; j < DU_MAXV4; ++j) {
        const int c = lane + 64 * j < nv ? lane + 64 * j : nv - 1;
        pe[j] = *reinterpret_cast<const uint2*>(wpe + (size_t)pos * D + c * 4);
    }
    // LayerNorm weights with the same batch (without the fused LayerNorm the lanes read the row's
    // own x, valid and unused, so that the loads need no branch)
    const float4* gsrc = reinterpret_cast<const float4*>(h ? ln_g : x + (size_t)b * ldx);
    const float4* bsrc = reinterpret_cast<const float4*>(h ? ln_b : x + (size_t)b * ldx);
    float4 lg[DU_MAXV4], lb[DU_MAXV4];
#pragma unroll
    for (int j = 0; j < DU_MAXV4; ++j) {
        const int c = lane + 64 * j < nv ? lane + 64 * j : nv - 1;
        lg[j] = gsrc[c];
        lb[j] = bsrc[c];
    }
    const unsigned long long best = wave_max_u64(
        key_rounds_from(keys, i, nparts, sb, sp, lane, 64 * KEY_ROUND, key_round_max(k0, nparts, lane, 0, 0ull)));

    int tok;
    if (!fin) {
        // best == 0 means no shard produced a candidate (cannot happen for vocab >= 1); stay in
        // bounds anyway by emitting EOS.
        tok = best ? (int)(~(unsigned int)(best & 0xffffffffull)) : eos;
        tok = (int)dlms_idx(tok, V, CHK_UPDATE_TOKEN);
    } else {
        tok = (int)dlms_idx(last_tok, V, CHK_UPDATE_TOKEN);
    }
    bool stop_hit = false;
    if constexpr (STOP) {
        const int j = lane & (STOP_MAX_LEN - 1);
        // elements past the sequence's end agree; the last one is the token chosen now (index
        // live_len, not yet in memory); the others were loaded above and lie at or past P
        const bool ok = st_m > 0 && (j >= st_m || (live_len + 1 - st_m >= st_P &&
                                                   (st_at == live_len ? tok : st_have) == st_tok));
        const unsigned int hits = (unsigned int)__ballot(ok);  // lanes 0..31: a byte per sequence
#pragma unroll
        for (int s = 0; s < STOP_MAX_SEQS; ++s) stop_hit = stop_hit || ((hits >> (8 * s)) & 0xffu) == 0xffu;
    }
    if (lane == 0) {
        if (!fin) {
            out_tokens[(size_t)b * max_len + live_len] = tok;
            atomicOr(seen + (size_t)b * seen_words + (tok >> 5), 1u << (tok & 31));  // no read-back wait
            lens[b] = live_len + 1;
            if (tok == eos || live_len + 1 >= max_len || (STOP && stop_hit)) finished[b] = 1;
        }
        cur_tok[b] = tok;
        cur_pos[b] = pos;
        cur_kvlen[b] = pos + 1;
    }
    const bf16_t* a = wte + (size_t)tok * D;
    float4* o = reinterpret_cast<float4*>(x + (size_t)b * ldx);
    float4 v[DU_MAXV4];
    uint2 te[DU_MAXV4];
#pragma unroll
    for (int j = 0; j < DU_MAXV4; ++j)
        te[j] = *reinterpret_cast<const uint2*>(a + (lane + 64 * j < nv ? lane + 64 * j : nv - 1) * 4);
#pragma unroll
    for (int j = 0; j < DU_MAXV4; ++j) {
        const int c = lane + 64 * j;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c >= nv) continue;
        const uint2 e = te[j];
        v[j] = make_float4(bf16_to_f32((bf16_t)(e.x & 0xffffu)) + bf16_to_f32((bf16_t)(pe[j].x & 0xffffu)),
                           bf16_to_f32((bf16_t)(e.x >> 16)) + bf16_to_f32((bf16_t)(pe[j].x >> 16)),
                           bf16_to_f32((bf16_t)(e.y & 0xffffu)) + bf16_to_f32((bf16_t)(pe[j].y & 0xffffu)),
                           bf16_to_f32((bf16_t)(e.y >> 16)) + bf16_to_f32((bf16_t)(pe[j].y >> 16)));
        o[c] = v[j];
    }
    if (h == nullptr) return;
    // layer 0's LN1 of the new row (the overlapped decode step then skips that launch): the same
    // statistics order as add_layernorm_kernel -- per-lane float4 sums, wave sums, two passes
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < DU_MAXV4; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    const float mean = wave_sum(s) / (float)D;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < DU_MAXV4; ++j) {
        if (lane + 64 * j < nv) {
            const float p = v[j].x - mean, q = v[j].y - mean, r = v[j].z - mean, t = v[j].w - mean;
            ss += (p * p + q * q) + (r * r + t * t);
        }
    }
    const float rstd = rsqrtf(wave_sum(ss) / (float)D + eps);
#pragma unroll
    for (int j = 0; j < DU_MAXV4; ++j) {
        const int c = lane + 64 * j;
        if (c >= nv) continue;
        const float4 g = lg[j], be = lb[j];
        uint2 pk;
        pk.x = pack_bf16x2((v[j].x - mean) * rstd * g.x + be.x, (v[j].y - mean) * rstd * g.y + be.y);
        pk.y = pack_bf16x2((v[j].z - mean) * rstd * g.z + be.z, (v[j].w - mean) * rstd * g.w + be.w);
        reinterpret_cast<uint2*>(h + (size_t)b * ldh)[c] = pk;
    }
}

extern "C" hipError_t dlms_embed(const int* tokens, const int* positions, const void* wte, const void* wpe, float* x,
                                 int ldx, int R, int D, int V, int P, hipStream_t stream) {
    if (D % 8 != 0 || R <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(embed_kernel, dim3((R + 3) / 4), dim3(256), 0, stream, tokens, positions,
                       reinterpret_cast<const bf16_t*>(wte), reinterpret_cast<const bf16_t*>(wpe), x, ldx, R, D, V, P);
    return hipGetLastError();
}

extern "C" hipError_t dlms_decode_update(const unsigned long long* keys, int nparts, long long sb, long long sp,
                                         const int* slot_map, int* lens, int* finished, int* out_tokens, int max_len,
                                         unsigned int* seen, int seen_words, int* cur_tok, int* cur_pos,
                                         int* cur_kvlen, const void* wte, const void* wpe, float* x, int ldx, int B,
                                         int D, int eos, int t_max, int n_slots, int V, const float* ln_g,
                                         const float* ln_b, float eps, void* h, int ldh, hipStream_t stream) {
    if (D % 8 != 0 || D > 64 * DU_MAXV4 * 4 || B <= 0 || nparts <= 0 || (h && (!ln_g || !ln_b || ldh % 4)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_update_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, stream, keys, nparts, sb, sp,
                       slot_map, lens, finished, out_tokens, max_len, seen, seen_words, cur_tok, cur_pos, cur_kvlen,
                       reinterpret_cast<const bf16_t*>(wte), reinterpret_cast<const bf16_t*>(wpe), x, ldx, B, D, eos,
                       t_max, n_slots, V, ln_g, ln_b, eps, reinterpret_cast<bf16_t*>(h), ldh, StopArgs<false>{});
    return hipGetLastError();
}

extern "C" hipError_t dlms_decode_update_stop(const unsigned long long* keys, int nparts, long long sb, long long sp,
                                              const int* slot_map, int* lens, int* finished, int* out_tokens,
                                              int max_len, unsigned int* seen, int seen_words, int* cur_tok,
                                              int* cur_pos, int* cur_kvlen, const void* wte, const void* wpe, float* x,
                                              int ldx, int B, int D, int eos, int t_max, int n_slots, int V,
                                              const float* ln_g, const float* ln_b, float eps, void* h, int ldh,
                                              const int* prompt_len, const int* stop_len, const int* stop_tok,
                                              hipStream_t stream) {
    if (D % 8 != 0 || D > 64 * DU_MAXV4 * 4 || B <= 0 || nparts <= 0 || (h && (!ln_g || !ln_b || ldh % 4)) ||
        !prompt_len || !stop_len || !stop_tok || max_len < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_update_kernel<true>, dim3((B + 3) / 4), dim3(256), 0, stream, keys, nparts, sb, sp,
                       slot_map, lens, finished, out_tokens, max_len, seen, seen_words, cur_tok, cur_pos, cur_kvlen,
                       reinterpret_cast<const bf16_t*>(wte), reinterpret_cast<const bf16_t*>(wpe), x, ldx, B, D, eos,
                       t_max, n_slots, V, ln_g, ln_b, eps, reinterpret_cast<bf16_t*>(h), ldh,
                       StopArgs<true>{prompt_len, stop_len, stop_tok});
    return hipGetLastError();
}

extern "C" hipError_t dlms_argmax_reduce(const unsigned long long* keys, int nparts, long long sb,
                                         unsigned long long* out, int B, hipStream_t stream) {
    if (B <= 0 || nparts <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(argmax_reduce_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, keys, nparts, sb, out, B);
    return hipGetLastError();
}

// Prefill bookkeeping on the device: set the repetition-penalty bit of every prompt token in its
// sequence's seen bitmap (rows pre-zeroed by the caller).  One thread per packed prompt token;
// duplicate tokens of a row OR the same bit, so the result does not depend on the order.
__global__ __launch_bounds__(256) void seen_set_kernel(const int* __restrict__ tokens, const int* __restrict__ rows,
                                                       int R, unsigned int* seen, int seen_words, int n_rows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const int t = tokens[i];
    if (t < 0 || (t >> 5) >= seen_words) {  // the host validates ids; never write out of the row
        dlms_idx(t, (long long)seen_words * 32, CHK_SEEN_TOKEN);
        return;
    }
    const size_t row = dlms_idx(rows[i], n_rows, CHK_SEEN_ROW);
    atomicOr(seen + row * seen_words + (t >> 5), 1u << (t & 31));
}

extern "C" hipError_t dlms_seen_set(const int* tokens, const int* rows, int R, unsigned int* seen, int seen_words,
                                    int n_rows, hipStream_t stream) {
    if (R <= 0 || seen_words <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seen_set_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, tokens, rows, R, seen, seen_words,
                       n_rows);
    return hipGetLastError();
}

// Prompt-prefix cache: broadcast the first pfx[i] key rows of the prefix store into KV-cache slot
// slots[i], for every layer, K and V, and head.  Cache [L][2][slots][H][t_max][row], store
// [L][2][H][cap][row] with row = 128 B (bf16) or 64 B (e4m3): per (slot, layer, k/v, head) one
// contiguous run of pfx * row bytes on both sides, moved as 16-byte chunks with plain stores.
// One workgroup per (layer * 2 + k/v, listed slot) loops over the heads' chunks.  slots / pfx are
// read on the device (the staged arrays of a captured prefill); pfx = 0 copies nothing.
__global__ __launch_bounds__(256) void kv_prefix_fill_kernel(unsigned char* __restrict__ kv,
                                                             const unsigned char* __restrict__ store,
                                                             const int* __restrict__ slots,
                                                             const int* __restrict__ pfx, int n_slots, int H,
                                                             int t_max, int cap, int row_bytes) {
    const int lk = blockIdx.x;
    const int i = blockIdx.y;
    const int lim = cap < t_max ? cap : t_max;
    int p = (int)dlms_idx(pfx[i], lim + 1, CHK_PFX_LEN);
    p = p < 0 ? 0 : (p > lim ? lim : p);  // never past the store's or the slot's rows
    const int s = slots[i];
    if (s < 0 || s >= n_slots) {  // the host validates slots; never write outside the cache
        dlms_idx(s, n_slots, CHK_PFX_SLOT);
        return;
    }
    const int per_head = p * (row_bytes >> 4);  // 16-byte chunks of one head's run
    const int total = H * per_head;
    const unsigned char* src = store + (size_t)lk * H * cap * row_bytes;
    unsigned char* dst = kv + ((size_t)lk * n_slots + s) * H * t_max * row_bytes;
    for (int c = threadIdx.x; c < total; c += 256) {
        const int h = c / per_head, rem = c - h * per_head;
        const uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)h * cap * row_bytes + (size_t)rem * 16);
        *reinterpret_cast<uint4*>(dst + (size_t)h * t_max * row_bytes + (size_t)rem * 16) = v;
    }
}

extern "C" hipError_t dlms_kv_prefix_fill(void* kv, const void* store, const int* slots, const int* pfx, int n,
                                          int layers2, int n_slots, int H, int t_max, int cap, int row_bytes,
                                          hipStream_t stream) {
    if (n <= 0 || layers2 <= 0 || n_slots <= 0 || H <= 0 || t_max <= 0 || cap <= 0 || n > 65535 ||
        (row_bytes != 64 && row_bytes != 128))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(kv_prefix_fill_kernel, dim3(layers2, n), dim3(256), 0, stream,
                       reinterpret_cast<unsigned char*>(kv), reinterpret_cast<const unsigned char*>(store), slots, pfx,
                       n_slots, H, t_max, cap, row_bytes);
    return hipGetLastError();
}

// Best of n: fork freshly prefilled slots into sibling slots.  For every pair i the first lens[i] key
// rows of slot src[i] go to slot dst[i], for every layer, K and V, and head: per (pair, layer, k/v,
// head) one contiguous run of lens * row bytes on both sides of the cache [L][2][slots][H][t_max][row]
// (row = 128 B bf16 or 64 B e4m3), moved as 16-byte chunks with plain loads and stores.  A unit is one
// (pair, layer * 2 + k/v); a capped grid strides over the units (768 children x 24 units at the
// serving shape: one workgroup per unit would be 18 k tiny workgroups), each workgroup looping over
// its unit's heads' chunks.  src / dst / lens are read on the device (the staged fork table of a
// captured prefill); lens = 0 and src == dst copy nothing, lengths are clamped to t_max, and a slot
// outside the cache writes nothing.  The host guarantees that no slot is both read and written and
// that no slot is written twice, so the workgroups never race; a parent may be read by many children.
#define KV_FORK_MAX_GRID 2048
__global__ __launch_bounds__(256) void kv_fork_kernel(unsigned char* __restrict__ kv, const int* __restrict__ src,
                                                      const int* __restrict__ dst, const int* __restrict__ lens,
                                                      int n, int layers2, int n_slots, int H, int t_max,
                                                      int row_bytes) {
    const int units = n * layers2;
    const size_t head_bytes = (size_t)t_max * row_bytes;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        const int i = u / layers2, lk = u - i * layers2;
        const int s = src[i], d = dst[i];
        if (s < 0 || s >= n_slots) {  // the host validates slots; never read or write outside the cache
            dlms_idx(s, n_slots, CHK_FORK_SRC);
            continue;
        }
        if (d < 0 || d >= n_slots) {
            dlms_idx(d, n_slots, CHK_FORK_DST);
            continue;
        }
        int p = (int)dlms_idx(lens[i], t_max + 1, CHK_FORK_LEN);
        p = p < 0 ? 0 : (p > t_max ? t_max : p);  // never past the slot's rows
        if (p == 0 || s == d) continue;
        const int per_head = p * (row_bytes >> 4);  // 16-byte chunks of one head's run
        const int total = H * per_head;
        const unsigned char* from = kv + ((size_t)lk * n_slots + s) * H * head_bytes;
        unsigned char* to = kv + ((size_t)lk * n_slots + d) * H * head_bytes;
        for (int c = threadIdx.x; c < total; c += 256) {
            const int h = c / per_head, rem = c - h * per_head;
            const size_t off = (size_t)h * head_bytes + (size_t)rem * 16;
            const uint4 v = *reinterpret_cast<const uint4*>(from + off);
            *reinterpret_cast<uint4*>(to + off) = v;
        }
    }
}

extern "C" hipError_t dlms_kv_fork(void* kv, const int* src, const int* dst, const int* lens, int n, int layers2,
                                   int n_slots, int H, int t_max, int row_bytes, hipStream_t stream) {
    if (n <= 0 || layers2 <= 0 || n_slots <= 0 || H <= 0 || t_max <= 0 || n > 65535 || layers2 > 4096 ||
        (row_bytes != 64 && row_bytes != 128) || (long long)H * t_max * (row_bytes >> 4) > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const int units = n * layers2;  // < 2^28
    hipLaunchKernelGGL(kv_fork_kernel, dim3(units < KV_FORK_MAX_GRID ? units : KV_FORK_MAX_GRID), dim3(256), 0,
                       stream, reinterpret_cast<unsigned char*>(kv), src, dst, lens, n, layers2, n_slots, H, t_max,
                       row_bytes);
    return hipGetLastError();
}

DLMS_CHECK_EXPORT(decode)
