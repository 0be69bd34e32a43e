// The log-probability of one token per row of f32 logits: what the decode reports for the token it
// just chose (decode mode), and what score() reports for a given next token (teacher-forced mode).
//
// Definition (normative; models/gpt2.py reference_logprob is the same in numpy float64):
//   l_j          = seen(j) ? (z_j < 0 ? z_j * penalty : z_j / penalty) : z_j        (f32, as in sample.hip)
//   m            = max_j l_j
//   logprob(tok) = (l_tok - m) - log( sum_{j < vocab} exp(l_j - m) )
// over the logits as the sampler sees them (logit_bans has stored -inf at the banned columns, which
// then contribute exp(-inf) = 0): the distribution that the logits processors leave, at temperature
// 1, ahead of top-k / top-p.  Columns >= vocab never take part, whatever they hold.  Teacher-forced
// mode: no bitmap, penalty 1 -- the model's raw distribution.
//
// One 1024-thread workgroup per row.  The row is read from memory ONCE, into registers, in the
// sampler's layout (float4 chunk t + 1024 j of thread t; unconditional loads at clamped indices,
// values masked by the column index afterwards); the maximum and then the sum of exponentials are
// reduced over the wave and through 16 LDS words each, in a fixed order (the result does not
// depend on timing: graph replays and eager runs agree bit for bit).  The thread that owns the
// token's column supplies l_tok; thread 0 stores the result.  Accumulation in f32: |error| < 5e-5
// for |l| <= 100 (rounding of l_j - m <= 2^-24 * 88 relative per term, expf a few ulp, the
// summation tree < 1e-5 relative on the sum, l_tok - m one ulp at 100).
//
// Decode mode: the token is the low word ~tok of the row's key, as the sampler wrote it; the row's
// slot b is the row index or slot_map[row]; the value goes to out[b][lens[b]] -- the index
// decode_update, which runs next and advances lens, writes the token to.  Nothing is read or
// written for a finished slot or for lens[b] >= max_length.
#include "common.h"

#define LPB_THREADS 1024
#define LPB_WAVES (LPB_THREADS / 64)

template <int NJ, bool DECODE>
__global__ __launch_bounds__(LPB_THREADS) void token_logprob_kernel(
    const float* __restrict__ logits, long long ldz, const unsigned int* __restrict__ seen, int seen_words,
    const unsigned long long* __restrict__ keys, long long ldk, const int* __restrict__ targets,
    const int* __restrict__ lens, const int* __restrict__ finished, const int* __restrict__ slot_map, int n_slots,
    float penalty, int vocab, int max_length, float* out, long long ldo) {
    __shared__ float red_max[LPB_WAVES];
    __shared__ float red_sum[LPB_WAVES];
    __shared__ float tok_l;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row = blockIdx.x;
    const int nv4 = (int)(ldz >> 2);

    // where the value goes and which token it is of (the same words in every lane)
    int tok;
    float* dst;
    if constexpr (DECODE) {
        const int b = slot_map ? (int)dlms_idx(slot_map[row], n_slots, CHK_LOGPROB_SLOT) : row;
        if (finished[b]) return;
        const int len = lens[b];
        if (len >= max_length) return;
        dst = out + (size_t)b * ldo + dlms_idx(len, max_length, CHK_LOGPROB_LEN);
        tok = (int)~(unsigned int)keys[(size_t)row * ldk];
    } else {
        dst = out + row;
        tok = targets[row];
    }
    tok = (int)dlms_idx(tok, vocab, CHK_LOGPROB_TOKEN);
    // (a token outside the vocabulary indexes nothing here: no thread owns its column, and the row's
    // value is NaN)
    const bool tok_ok = tok >= 0 && tok < vocab;

    // ---- the row into registers (sample.hip's layout)
    const float4* zrow = reinterpret_cast<const float4*>(logits + (size_t)row * ldz);
    float4 z[NJ];
    unsigned int sw[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = t + LPB_THREADS * j;
        const int ic = i < nv4 ? i : nv4 - 1;
        z[j] = zrow[ic];
        if constexpr (DECODE) {
            const int w = ic >> 3;  // 4 columns of a chunk share one 32-column bitmap word
            sw[j] = seen[(size_t)row * seen_words + (w < seen_words ? w : seen_words - 1)];
        } else {
            sw[j] = 0u;
        }
    }
    // Element (j, e) is column 4 t + 4096 j + e: it exists iff 4096 j + e < vrem
    const int vrem = vocab - 4 * t;
    const int trem = tok - 4 * t;  // the token is element (j, e) of this thread iff 4096 j + e == trem
    float l[NJ][4];
    float tmax = -INFINITY, mine = 0.f;
    bool owner = false;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float v4[4] = {z[j].x, z[j].y, z[j].z, z[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int off = 4 * LPB_THREADS * j + e;
            float v = v4[e];
            if (DECODE && ((sw[j] >> ((4 * t + off) & 31)) & 1u)) v = v < 0.f ? v * penalty : v / penalty;
            v = off < vrem ? v : -INFINITY;  // a select: whatever a column >= vocab holds (NaN too) is dropped
            l[j][e] = v;
            tmax = fmaxf(tmax, v);
            if (off == trem) {
                owner = true;
                mine = v;
            }
        }
    }
    if (owner && tok_ok) tok_l = mine;

    // ---- m: waves, then 16 words
    const float wmax = wave_max(tmax);
    if (lane == 0) red_max[wave] = wmax;
    __syncthreads();
    float m = red_max[0];
#pragma unroll
    for (int w = 1; w < LPB_WAVES; ++w) m = fmaxf(m, red_max[w]);

    // ---- the sum of exponentials (a dropped or banned column: exp(-inf) = 0)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += expf(l[j][e] - m);
    const float wsum = wave_sum(s);
    if (lane == 0) red_sum[wave] = wsum;
    __syncthreads();
    if (t == 0) {
        float total = 0.f;
#pragma unroll
        for (int w = 0; w < LPB_WAVES; ++w) total += red_sum[w];
        *dst = tok_ok ? (tok_l - m) - logf(total) : __int_as_float(0x7fc00000);
    }
}

// logits [B][ldz] f32 (columns >= vocab ignored).  Decode mode (targets == nullptr): seen
// [B][seen_words] rows parallel to the logits rows, keys [B][ldk] (column 0 read), lens / finished
// indexed by the row's slot (row i, or slot_map[i]), out [slots][ldo] with ldo >= max_length.
// Teacher-forced mode (targets [B] int32): out [B]; every other state pointer must be null.
extern "C" hipError_t dlms_token_logprob(const float* logits, long long ldz, const unsigned int* seen, int seen_words,
                                         const unsigned long long* keys, long long ldk, const int* targets,
                                         const int* lens, const int* finished, const int* slot_map, int n_slots,
                                         float penalty, int vocab, int max_length, float* out, long long ldo, int B,
                                         hipStream_t stream) {
    if (B <= 0 || vocab < 1 || vocab > 65536 || ldz < vocab || ldz % 4 || ldz > 4ll * LPB_THREADS * 16 ||
        logits == nullptr || ((uintptr_t)logits & 15) || out == nullptr || ((uintptr_t)out & 3))
        return hipErrorInvalidValue;
    const bool decode = targets == nullptr;
    if (decode) {
        if (seen == nullptr || keys == nullptr || lens == nullptr || finished == nullptr || ldk < 1 ||
            seen_words * 32ll < vocab || !(penalty > 0.f) || max_length < 1 || ldo < max_length ||
            (slot_map != nullptr && n_slots < 1))
            return hipErrorInvalidValue;
    } else if (seen != nullptr || keys != nullptr || lens != nullptr || finished != nullptr || slot_map != nullptr ||
               penalty != 1.f) {
        return hipErrorInvalidValue;
    }
    const int nv4 = (int)(ldz / 4);
#define LPB_LAUNCH(NJ)                                                                                          \
    do {                                                                                                        \
        if (decode)                                                                                             \
            hipLaunchKernelGGL((token_logprob_kernel<NJ, true>), dim3(B), dim3(LPB_THREADS), 0, stream, logits, \
                               ldz, seen, seen_words, keys, ldk, targets, lens, finished, slot_map, n_slots,    \
                               penalty, vocab, max_length, out, ldo);                                           \
        else                                                                                                    \
            hipLaunchKernelGGL((token_logprob_kernel<NJ, false>), dim3(B), dim3(LPB_THREADS), 0, stream,        \
                               logits, ldz, seen, seen_words, keys, ldk, targets, lens, finished, slot_map,     \
                               n_slots, penalty, vocab, max_length, out, ldo);                                  \
    } while (0)
    if (nv4 <= LPB_THREADS * 1) LPB_LAUNCH(1);
    else if (nv4 <= LPB_THREADS * 4) LPB_LAUNCH(4);
    else if (nv4 <= LPB_THREADS * 13) LPB_LAUNCH(13);  // GPT-2: 50304 padded columns
    else LPB_LAUNCH(16);
#undef LPB_LAUNCH
    return hipGetLastError();
}

DLMS_CHECK_EXPORT(logprob)
