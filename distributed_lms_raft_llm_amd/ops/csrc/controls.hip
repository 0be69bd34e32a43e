// Generation controls on the device (models/config.py GenerationControls): n-gram blocking and a
// minimum length as bans on the f32 logits between the LM head and the sampler (logit_bans, this
// file), stop sequences in the bookkeeping of the chosen token (decode.hip, decode_update_kernel
// with STOP).  Both run inside the replayed decode and prefill graphs, like the sampler.
//
// Definition (normative; models/gpt2.py banned_tokens / stop_hit are the same in Python; the bans
// are HF's NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor).  Let seq be the
// row's tokens so far, prompt included, L its length and P the prompt length.
//   n-gram ban   if L + 1 >= n, ban seq[i+n-1] for every 0 <= i <= L-n with
//                seq[i : i+n-1] == seq[L-n+1 : L].  With n = 1 every token of seq is banned.  This
//                applies to the first generated token too, the one the prefill's LM head picks.
//   minimum      while L - P < min_new_tokens, EOS is banned.
//   banned       a banned token's f32 logit becomes -inf before the penalty.  After that the
//                definition in sample.hip applies word for word.  Greedy decoding with bans is that
//                definition at top_k = 1: the largest key (f32_ordered(l) << 32) | ~j, with ties
//                going to the lower id.
//   stop         after a token is written at index p, the row finishes if for some stop sequence s
//                of length m both hold: p + 1 - m >= P, and seq[p+1-m : p+1] == s.  The match lies
//                wholly in generated tokens.  The stop tokens stay in the returned sequence, as EOS
//                does.  EOS and max_length stop a row as before.
//
// logit_bans: one 256-thread workgroup per row.  The row's state words (length, stop flag, prompt
// length) and its whole token row out_tokens[0 : max_len) are requested together -- the token loads
// do not wait for the length: every thread reads its strided share of max_len tokens, whatever
// the row holds, into LDS -- so the kernel is one memory round trip (two through a slot map) and
// then LDS compares.  Thread i tests start i of an earlier (n-1)-gram against the row's last
// n - 1 tokens and stores -inf at the token that followed it; several threads may store the same
// -inf to one column (plain stores, no atomics, no order needed).  A finished row is left alone.
// Rows map to slots directly or through slot_map, exactly as the sampler's lens / streams do.
#include "common.h"

#define BAN_THREADS 256

__global__ __launch_bounds__(BAN_THREADS) void logit_bans_kernel(
    float* logits, long long ldz, const int* __restrict__ lens, const int* __restrict__ finished,
    const int* __restrict__ prompt_len, const int* __restrict__ out_tokens, long long ldt, int max_len,
    const int* __restrict__ slot_map, int n_slots, int ngram, int min_new, int eos, int vocab) {
    extern __shared__ int seq[];  // [max_len]
    const int t = threadIdx.x;
    const int row = blockIdx.x;
    const int b = slot_map ? (int)dlms_idx(slot_map[row], n_slots, CHK_BANS_SLOT) : row;
    // the row's state and tokens in one batch (every thread reads the same three words)
    const int len0 = lens[b];
    const int fin = finished[b];
    const int P = prompt_len[b];
    const int* trow = out_tokens + (size_t)b * ldt;
    for (int i = t; i < max_len; i += BAN_THREADS) seq[i] = trow[i];
    if (fin) return;  // (the whole workgroup: the condition is the row's)
    int L = (int)dlms_idx(len0, (long long)max_len + 1, CHK_BANS_LEN);
    L = L < 0 ? 0 : (L > max_len ? max_len : L);  // never past the LDS row
    __syncthreads();
    float* z = logits + (size_t)row * ldz;
    const float ninf = -__builtin_inff();
    if (ngram > 0) {
        const int suf = L - ngram + 1;  // where the row's last n - 1 tokens start (>= 0 when the loop runs)
        for (int i = t; i <= L - ngram; i += BAN_THREADS) {
            bool eq = true;
            for (int j = 0; j < ngram - 1 && eq; ++j) eq = seq[i + j] == seq[suf + j];
            const int tok = seq[i + ngram - 1];
            if (eq && tok >= 0 && tok < vocab) z[tok] = ninf;  // (ids are validated at admission; stay in the row)
        }
    }
    if (t == 0 && L - P < min_new && eos >= 0 && eos < vocab) z[eos] = ninf;
}

extern "C" hipError_t dlms_logit_bans(float* logits, long long ldz, const int* lens, const int* finished,
                                      const int* prompt_len, const int* out_tokens, long long ldt, int max_len,
                                      const int* slot_map, int n_slots, int ngram, int min_new, int eos, int vocab,
                                      int rows, hipStream_t stream) {
    if (rows <= 0 || max_len < 1 || max_len > 12288 || vocab < 1 || ldz < vocab || ldt < max_len || ngram < 0 ||
        min_new < 0 || !logits || !lens || !finished || !prompt_len || !out_tokens)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(logit_bans_kernel, dim3(rows), dim3(BAN_THREADS), (size_t)max_len * sizeof(int), stream, logits,
                       ldz, lens, finished, prompt_len, out_tokens, ldt, max_len, slot_map, n_slots, ngram, min_new,
                       eos, vocab);
    return hipGetLastError();
}

DLMS_CHECK_EXPORT(controls)
