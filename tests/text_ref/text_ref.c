/* TEST INFRASTRUCTURE: a plain-C restatement of the TEXT SEARCH rules a-g of include/lynse_hip.h (InvertedTextIndex::search,
 * src/engine.rs:927-1054), document at a time the way the reference loops (:1020-1050), with the pinned slot order and libm's logf.
 * Built with -ffp-contract=off -fno-fast-math by tests/text_common.py; it shares no code with the library.
 *
 * The corpus comes document-major: doc_ptr u64[n + 1], doc_term u32 ascending within a document, doc_tf u32, doc_len u32[n]. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

static uint64_t sat_mul(uint64_t a, uint64_t b) {
    if (a == 0 || b == 0) return 0;
    return a > UINT64_MAX / b ? UINT64_MAX : a * b;
}

/* the frequency of `term` in document d, 0 when absent */
static uint32_t tf_of(const uint64_t *doc_ptr, const uint32_t *doc_term, const uint32_t *doc_tf, uint64_t d, uint32_t term) {
    uint64_t lo = doc_ptr[d], hi = doc_ptr[d + 1];
    while (lo < hi) {
        uint64_t mid = lo + (hi - lo) / 2;
        if (doc_term[mid] < term) lo = mid + 1;
        else if (doc_term[mid] > term) hi = mid;
        else return doc_tf[mid];
    }
    return 0;
}

/* rules b, d, e: avg, the weights and the candidate flags from the live statistics */
void tr_weights(uint64_t docs, uint64_t total, const uint64_t *df, const uint32_t *count, uint32_t T, uint32_t k, float *avg, float *w,
                uint32_t *cand) {
    *avg = 1.0f;
    for (uint32_t t = 0; t < T; ++t) {
        w[t] = 0.0f;
        cand[t] = 0;
    }
    if (docs == 0) return;
    float n_docs = (float)docs;
    float a = (float)total / (float)docs;
    *avg = a > 1.0f ? a : 1.0f;
    int have = 0;
    uint64_t min_df = 0;
    for (uint32_t t = 0; t < T; ++t)
        if (df[t] > 0 && (!have || df[t] < min_df)) {
            min_df = df[t];
            have = 1;
        }
    if (!have) return;
    uint64_t c1 = sat_mul(min_df, 4), c2 = sat_mul((uint64_t)k, 8);
    uint64_t cutoff = c1 > c2 ? c1 : c2;
    int any = 0;
    for (uint32_t t = 0; t < T; ++t) {
        if (df[t] == 0) continue;
        if (df[t] < docs && df[t] <= cutoff) {
            cand[t] = 1;
            any = 1;
        }
        float d = (float)df[t];
        float x = n_docs - d;
        x = x + 0.5f;
        float y = d + 0.5f;
        float r = x / y;
        r = r + 1.0f;
        float idf = logf(r);
        w[t] = (float)count[t] * idf;
    }
    if (!any)
        for (uint32_t t = 0; t < T; ++t)
            if (df[t] > 0) cand[t] = 1;
}

/* One query over the whole corpus.  live: u8[n] or NULL (every row).  Outputs: score f32[n] (the rule-f sum of every live row, in
 * slot order or, with reversed != 0, in reverse slot order), result u8[n] (rule g), matched u8[n] (query terms the row holds, capped
 * at 255), stats u64[2 + T] = docs, total, df of every slot.  Returns the number of results. */
uint64_t tr_search(const uint32_t *doc_len, const uint64_t *doc_ptr, const uint32_t *doc_term, const uint32_t *doc_tf, uint64_t n,
                   const uint8_t *live, const uint32_t *q_terms, const uint32_t *q_counts, uint32_t T, uint32_t k, int reversed, float *score,
                   uint8_t *result, uint8_t *matched, uint64_t *stats, float *w, uint32_t *cand) {
    uint64_t docs = 0, total = 0, passed = 0;
    memset(result, 0, n);
    memset(matched, 0, n);
    for (uint64_t d = 0; d < n; ++d) score[d] = 0.0f;
    for (uint32_t t = 0; t < T; ++t) stats[2 + t] = 0;
    for (uint64_t d = 0; d < n; ++d) {
        if (live && !live[d]) continue;
        docs += 1;
        total += doc_len[d];
        for (uint32_t t = 0; t < T; ++t)
            if (tf_of(doc_ptr, doc_term, doc_tf, d, q_terms[t]) > 0) stats[2 + t] += 1;
    }
    stats[0] = docs;
    stats[1] = total;
    float avg;
    tr_weights(docs, total, stats + 2, q_counts, T, k, &avg, w, cand);
    if (docs == 0 || k == 0) return 0;
    const float k1 = 1.2f, b = 0.75f;
    const float K = k1 + 1.0f;
    for (uint64_t d = 0; d < n; ++d) {
        if (live && !live[d]) continue;
        float s = 0.0f;
        int is_cand = 0;
        unsigned m = 0;
        for (uint32_t i = 0; i < T; ++i) {
            uint32_t t = reversed ? T - 1 - i : i;
            uint32_t tfi = tf_of(doc_ptr, doc_term, doc_tf, d, q_terms[t]);
            if (tfi == 0 || stats[2 + t] == 0) continue;
            m += 1;
            if (cand[t]) is_cand = 1;
            float tf = (float)tfi, dl = (float)doc_len[d];
            float bd = b * dl;
            float frac = bd / avg;
            float in = (1.0f - b) + frac;
            float scaled = k1 * in;
            float denom = tf + scaled;
            float num = tf * K;
            float top = w[t] * num;
            float term = top / denom;
            s = s + term;
        }
        score[d] = s;
        matched[d] = m > 255 ? 255 : (uint8_t)m;
        if (is_cand && s > 0.0f) {
            result[d] = 1;
            passed += 1;
        }
    }
    return passed;
}
