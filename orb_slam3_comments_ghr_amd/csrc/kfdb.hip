// kfdb.hip — KeyFrameDatabase on gfx950: steps 1 and 2 of DetectNBestCandidates
// (ref:src/KeyFrameDatabase.cc:669-770) and DetectRelocalizationCandidates (:920-974).
//
// The reference walks the query's words in ascending order and, per word, the inverted file's list of
// KeyFrames, changing mnPlaceRecognitionQuery / Words per hit.  For an entry with h >= 1 common words the
// walk has a closed form in the entry's state at entry to the call:
//     query != qid, not connected : query = qid, words = h, appended to lKFsSharingWords
//     query != qid, connected     : words = 1 (reset to 0 at every hit, then incremented)
//     query == qid                : words += h
// (relocalisation has no connected case), and the list is in first-visit order: ascending (first common
// word, position in the add sequence), because add() appends a KeyFrame to all of its words' lists at
// once.  So no inverted file is kept on the device: every entry's sorted word list is intersected with
// the query's, one wave per entry.
//
// Storage: entries live in slots in add order (a slot is never reused; an erased one is flagged dead),
// their words and values back to back in two pools that grow geometrically.  A query is three launches:
//     k_kfdb_count      per entry: common words, first common word, the state update; per workgroup the
//                       largest listed count and the number listed
//     k_kfdb_threshold  one workgroup: maxCommonWords, minCommonWords, and the entries above it
//                       compacted in slot order (a second small launch instead of a last-arriver merge)
//     k_kfdb_score      per scored entry: its rank in list order and L1Scoring::score
//                       (ref:Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), the terms formed by the
//                       lanes, their sum taken in ascending word order
// No floating-point atomics, no cross-workgroup hand-off inside a launch.  Built with -ffp-contract=off.
#include <climits>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/osg_dbow.h"
#include "kfdb_select.h"
#include "osg_internal.h"

namespace {

constexpr int QT = 256;          // threads per workgroup of the count and score kernels
constexpr int WPB = QT / 64;     // entries per workgroup: one per wave
constexpr int Q_STAGE = 4096;    // query words staged in LDS (16 KiB); longer queries are read from global
constexpr int TT = 1024;         // threads of the threshold workgroup

// index of w in the ascending q[0..nq), or -1
__device__ __forceinline__ int find_word(const int32_t *q, int nq, int32_t w)
{
    int lo = 0, hi = nq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q[mid] < w)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < nq && q[lo] == w) ? lo : -1;
}

template <bool STAGED>
__global__ __launch_bounds__(QT) void k_kfdb_count(int nslots, const int32_t *__restrict__ word,
                                                   const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                   const int32_t *__restrict__ alive,
                                                   const int32_t *__restrict__ qword, int nq, int which, int64_t qid,
                                                   const int32_t *__restrict__ conn, int nconn,
                                                   int64_t *__restrict__ st_query, int32_t *__restrict__ st_words,
                                                   int32_t *__restrict__ listed, int32_t *__restrict__ first,
                                                   int32_t *__restrict__ wg_max, int32_t *__restrict__ wg_cnt)
{
    __shared__ int32_t sq[STAGED ? Q_STAGE : 1];
    __shared__ int32_t s_h[WPB];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (STAGED) {
        for (int i = tid; i < nq; i += QT) sq[i] = qword[i];
        __syncthreads();
    }
    const int32_t *q = STAGED ? sq : qword;
    const int slot = blockIdx.x * WPB + wave;
    int lh = 0;
    if (slot < nslots) {
        int h = 0;
        int32_t fw = INT_MAX;
        if (alive[slot]) {
            const int64_t o = off[slot];
            const int n = len[slot];
            for (int i = lane; i < n; i += 64) {
                const int32_t w = word[o + i];
                if (find_word(q, nq, w) >= 0) {
                    h++;
                    fw = min(fw, w);
                }
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            h += __shfl_xor(h, d);
            fw = min(fw, __shfl_xor(fw, d));
        }
        if (lane == 0) {
            if (h > 0) {
                if (st_query[slot] != qid) {
                    bool connected = false;
                    if (which == OSG_KFDB_PLACE) connected = find_word(conn, nconn, slot) >= 0;
                    if (connected) {
                        st_words[slot] = 1;
                    } else {
                        st_query[slot] = qid;
                        st_words[slot] = h;
                        lh = h;
                    }
                } else {
                    st_words[slot] += h;
                }
            }
            listed[slot] = lh;
            first[slot] = fw;
        }
    }
    if (lane == 0) s_h[wave] = lh;
    __syncthreads();
    if (tid == 0) {
        int m = 0, c = 0;
        for (int k = 0; k < WPB; k++) {
            m = max(m, s_h[k]);
            c += s_h[k] > 0;
        }
        wg_max[blockIdx.x] = m;
        wg_cnt[blockIdx.x] = c;
    }
}

// hdr = {n_sharing, maxCommonWords, minCommonWords, n_scored}; scored[0..n_scored): slots, ascending
__global__ __launch_bounds__(TT) void k_kfdb_threshold(int nslots, int nwg, const int32_t *__restrict__ wg_max,
                                                       const int32_t *__restrict__ wg_cnt,
                                                       const int32_t *__restrict__ listed, int32_t *__restrict__ hdr,
                                                       int32_t *__restrict__ scored)
{
    __shared__ int32_t s_m[TT / 64], s_c[TT / 64], s_res[2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int m = 0, c = 0;
    for (int i = tid; i < nwg; i += TT) {
        m = max(m, wg_max[i]);
        c += wg_cnt[i];
    }
    for (int d = 32; d >= 1; d >>= 1) {
        m = max(m, __shfl_xor(m, d));
        c += __shfl_xor(c, d);
    }
    if (lane == 0) {
        s_m[wave] = m;
        s_c[wave] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int mm = 0, cc = 0;
        for (int k = 0; k < TT / 64; k++) {
            mm = max(mm, s_m[k]);
            cc += s_c[k];
        }
        s_res[0] = mm;
        s_res[1] = cc;
    }
    __syncthreads();
    const int maxw = s_res[0], nshare = s_res[1];
    const int minw = (int)((float)maxw * 0.8f);  // int minCommonWords = maxCommonWords * 0.8f
    __syncthreads();
    int base = 0;
    for (int b = 0; b < nslots; b += TT) {
        const int slot = b + tid;
        const bool f = slot < nslots && listed[slot] > minw;
        const unsigned long long mask = __ballot(f);
        if (lane == 0) s_c[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < TT / 64; k++) {
            const int v = s_c[k];
            before += k < wave ? v : 0;
            total += v;
        }
        if (f) scored[base + before + __popcll(mask & ((1ull << lane) - 1ull))] = slot;
        base += total;
        __syncthreads();
    }
    if (tid == 0) {
        hdr[0] = nshare;
        hdr[1] = maxw;
        hdr[2] = minw;
        hdr[3] = base;
    }
}

template <bool STAGED>
__global__ __launch_bounds__(QT) void k_kfdb_score(const int32_t *__restrict__ hdr, const int32_t *__restrict__ scored,
                                                   const int32_t *__restrict__ word, const double *__restrict__ value,
                                                   const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                   const int32_t *__restrict__ qword,
                                                   const double *__restrict__ qvalue, int nq,
                                                   const int32_t *__restrict__ first,
                                                   const int32_t *__restrict__ listed, float *__restrict__ st_score,
                                                   int32_t *__restrict__ o_slot, int32_t *__restrict__ o_words,
                                                   float *__restrict__ o_score, double *__restrict__ o_score64)
{
    __shared__ int32_t sq[STAGED ? Q_STAGE : 1];
    const int nsc = hdr[3];
    if ((int)blockIdx.x * WPB >= nsc) return;  // uniform over the workgroup
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (STAGED) {
        for (int i = tid; i < nq; i += QT) sq[i] = qword[i];
        __syncthreads();
    }
    const int32_t *q = STAGED ? sq : qword;
    const int idx = blockIdx.x * WPB + wave;
    if (idx >= nsc) return;  // uniform over the wave; no barrier below
    const int slot = scored[idx];
    // position in lKFsSharingWords order among the scored: ascending (first common word, slot)
    const int32_t fi = first[slot];
    int rank = 0;
    for (int j = lane; j < nsc; j += 64) {
        const int sj = scored[j];
        const int32_t fj = first[sj];
        rank += (fj < fi || (fj == fi && sj < slot)) ? 1 : 0;
    }
    for (int d = 32; d >= 1; d >>= 1) rank += __shfl_xor(rank, d);
    // L1Scoring::score: score += fabs(vi - wi) - fabs(vi) - fabs(wi) over the common words, ascending
    const int64_t o = off[slot];
    const int n = len[slot];
    double score = 0;
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        double t = 0;
        bool hit = false;
        if (i < n) {
            const int k = find_word(q, nq, word[o + i]);
            if (k >= 0) {
                const double vi = qvalue[k], wi = value[o + i];
                t = fabs(vi - wi) - fabs(vi) - fabs(wi);
                hit = true;
            }
        }
        unsigned long long mask = __ballot(hit);
        // every lane takes the same sum, term by term in lane (= word) order
        while (mask) {
            const int src = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            score += __shfl(t, src);
        }
    }
    if (lane == 0) {
        const double s64 = -score / 2.0;
        const float si = (float)s64;
        st_score[slot] = si;
        o_slot[rank] = slot;
        o_words[rank] = listed[slot];
        o_score[rank] = si;
        o_score64[rank] = s64;
    }
}

// one add: the pinned block {state, values, words} into the pools and the slot's record
__global__ __launch_bounds__(256) void k_kfdb_add(const osg_kfdb_state *__restrict__ st,
                                                  const double *__restrict__ src_value,
                                                  const int32_t *__restrict__ src_word, int n, int slot, int64_t o,
                                                  int32_t *__restrict__ word, double *__restrict__ value,
                                                  int64_t *__restrict__ off, int32_t *__restrict__ len,
                                                  int32_t *__restrict__ alive, int64_t *__restrict__ pq,
                                                  int32_t *__restrict__ pw, float *__restrict__ ps,
                                                  int64_t *__restrict__ rq, int32_t *__restrict__ rw,
                                                  float *__restrict__ rs)
{
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        word[o + i] = src_word[i];
        value[o + i] = src_value[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        off[slot] = o;
        len[slot] = n;
        alive[slot] = 1;
        pq[slot] = st->place_query;
        pw[slot] = st->place_words;
        ps[slot] = st->place_score;
        rq[slot] = st->reloc_query;
        rw[slot] = st->reloc_words;
        rs[slot] = st->reloc_score;
    }
}

// state_get / state_set between the pinned block and the slots (validated, and distinct for a set)
__global__ __launch_bounds__(256) void k_kfdb_state(int n, const int32_t *__restrict__ slots, int set,
                                                    int64_t *__restrict__ st_query, int32_t *__restrict__ st_words,
                                                    float *__restrict__ st_score, int64_t *__restrict__ h_query,
                                                    int32_t *__restrict__ h_words, float *__restrict__ h_score)
{
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int s = slots[i];
        if (set) {
            st_query[s] = h_query[i];
            st_words[s] = h_words[i];
            st_score[s] = h_score[i];
        } else {
            h_query[i] = st_query[s];
            h_words[i] = st_words[s];
            h_score[i] = st_score[s];
        }
    }
}

size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace

struct osg_kfdb {
    std::mutex mu;
    int device = 0;
    int32_t voc_words = 0;
    // host mirror of the slot records
    std::vector<int32_t> slot_of_entry;  // per entry id ever returned; -1 once erased
    std::vector<int32_t> entry_of_slot, map_of_slot, len_of_slot;
    std::vector<uint8_t> alive;
    int32_t n_live = 0;
    int64_t pool_used = 0;
    // device
    int64_t pool_cap = 0;
    int32_t *d_word = nullptr;
    double *d_value = nullptr;
    int32_t slot_cap = 0;
    int64_t *d_off = nullptr;
    int32_t *d_len = nullptr, *d_alive = nullptr;
    int64_t *d_q[2] = {};
    int32_t *d_w[2] = {};
    float *d_s[2] = {};
    int32_t nslots() const { return (int32_t)entry_of_slot.size(); }
};

namespace {

// a larger buffer with the first `keep` bytes of the old one
template <class T>
int regrow(osg_ctx *ctx, T *&p, size_t keep, size_t bytes)
{
    T *np = nullptr;
    if (hipMalloc((void **)&np, bytes) != hipSuccess)
        return osg_set_error(ctx, OSG_E_NOMEM, "keyframe database: device alloc %zu B failed", bytes);
    if (p && keep) {
        const hipError_t e = hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            (void)hipFree(np);
            return osg_set_error(ctx, OSG_E_HIP, "keyframe database: device copy failed");
        }
    }
    if (p) (void)hipFree(p);
    p = np;
    return OSG_OK;
}

int reserve(osg_ctx *ctx, osg_kfdb *db, int64_t add_words)
{
    if (db->pool_used + add_words > db->pool_cap) {
        const int64_t cap = std::max<int64_t>(2 * db->pool_cap, std::max<int64_t>(db->pool_used + add_words, 1 << 16));
        OSG_RC(regrow(ctx, db->d_word, 4 * (size_t)db->pool_used, 4 * (size_t)cap));
        OSG_RC(regrow(ctx, db->d_value, 8 * (size_t)db->pool_used, 8 * (size_t)cap));
        db->pool_cap = cap;
    }
    const int32_t ns = db->nslots();
    if (ns + 1 > db->slot_cap) {
        OSG_REQUIRE(ctx, ns < (1 << 30), "keyframe database: too many entries");
        const int32_t cap = std::max<int32_t>(2 * db->slot_cap, 1024);
        OSG_RC(regrow(ctx, db->d_off, 8 * (size_t)ns, 8 * (size_t)cap));
        OSG_RC(regrow(ctx, db->d_len, 4 * (size_t)ns, 4 * (size_t)cap));
        OSG_RC(regrow(ctx, db->d_alive, 4 * (size_t)ns, 4 * (size_t)cap));
        for (int k = 0; k < 2; k++) {
            OSG_RC(regrow(ctx, db->d_q[k], 8 * (size_t)ns, 8 * (size_t)cap));
            OSG_RC(regrow(ctx, db->d_w[k], 4 * (size_t)ns, 4 * (size_t)cap));
            OSG_RC(regrow(ctx, db->d_s[k], 4 * (size_t)ns, 4 * (size_t)cap));
        }
        db->slot_cap = cap;
    }
    return OSG_OK;
}

// strictly ascending word ids below the vocabulary's word count
int check_bow(osg_ctx *ctx, const osg_kfdb *db, int32_t n, const int32_t *word, const double *value)
{
    OSG_REQUIRE(ctx, n >= 0 && (n == 0 || (word && value)), "BowVector arrays");
    for (int32_t i = 0; i < n; i++) {
        OSG_REQUIRE(ctx, word[i] >= 0 && word[i] < db->voc_words, "word %d: id %d outside the vocabulary's %d words", i,
                    word[i], db->voc_words);
        OSG_REQUIRE(ctx, i == 0 || word[i] > word[i - 1], "word %d: ids are not strictly ascending", i);
    }
    return OSG_OK;
}

int same_device(osg_ctx *ctx, const osg_kfdb *db)
{
    OSG_REQUIRE(ctx, ctx->device == db->device, "the database lives on device %d, the context on %d", db->device,
                ctx->device);
    return OSG_OK;
}

void clear_locked(osg_kfdb *db)
{
    for (int32_t e : db->entry_of_slot) db->slot_of_entry[e] = -1;
    db->entry_of_slot.clear();
    db->map_of_slot.clear();
    db->len_of_slot.clear();
    db->alive.clear();
    db->n_live = 0;
    db->pool_used = 0;
}

int state_io(osg_ctx *ctx, osg_kfdb *db, int32_t which, int32_t n, const int32_t *entry, int64_t *query, int32_t *words,
             float *score, bool set)
{
    if (!ctx || !db) return OSG_E_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    OSG_RC(same_device(ctx, db));
    OSG_REQUIRE(ctx, which == OSG_KFDB_PLACE || which == OSG_KFDB_RELOC, "detector %d", which);
    OSG_REQUIRE(ctx, n >= 0 && (n == 0 || (entry && query && words && score)), "state arrays");
    if (n == 0) return OSG_OK;
    const size_t o_q = 0, o_sl = pad256(8 * (size_t)n), o_w = o_sl + pad256(4 * (size_t)n),
                 o_s = o_w + pad256(4 * (size_t)n), total = o_s + pad256(4 * (size_t)n);
    char *pin = (char *)osg_pinned(ctx, total);
    if (!pin) return osg_set_error(ctx, OSG_E_NOMEM, "pinned alloc failed");
    OSG_RC(osg_idle(ctx));
    int32_t *p_slot = (int32_t *)(pin + o_sl);
    std::vector<uint8_t> seen(set ? db->nslots() : 0, 0);
    for (int32_t i = 0; i < n; i++) {
        const int32_t e = entry[i];
        OSG_REQUIRE(ctx, e >= 0 && e < (int32_t)db->slot_of_entry.size() && db->slot_of_entry[e] >= 0,
                    "entry %d is not in the database", e);
        const int32_t s = db->slot_of_entry[e];
        if (set) {
            OSG_REQUIRE(ctx, !seen[s], "entry %d is set twice", e);
            seen[s] = 1;
        }
        p_slot[i] = s;
    }
    if (set) {
        std::memcpy(pin + o_q, query, 8 * (size_t)n);
        std::memcpy(pin + o_w, words, 4 * (size_t)n);
        std::memcpy(pin + o_s, score, 4 * (size_t)n);
    }
    const int blocks = std::min((n + 255) / 256, 1024);
    hipLaunchKernelGGL(k_kfdb_state, dim3(blocks), dim3(256), 0, ctx->stream, n, p_slot, set ? 1 : 0, db->d_q[which],
                       db->d_w[which], db->d_s[which], (int64_t *)(pin + o_q), (int32_t *)(pin + o_w),
                       (float *)(pin + o_s));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(osg_wait(ctx));
    if (!set) {
        std::memcpy(query, pin + o_q, 8 * (size_t)n);
        std::memcpy(words, pin + o_w, 4 * (size_t)n);
        std::memcpy(score, pin + o_s, 4 * (size_t)n);
    }
    return OSG_OK;
}

}  // namespace

extern "C" {

int osg_kfdb_create(osg_ctx *ctx, const osg_vocabulary *voc, osg_kfdb **out)
{
    if (!ctx) return OSG_E_INVALID;
    OSG_REQUIRE(ctx, voc && out, "null argument");
    *out = nullptr;
    int32_t nw = 0, scoring = 0;
    osg_vocabulary_words_scoring(voc, &nw, &scoring);
    if (scoring != OSG_S_L1)
        return osg_set_error(ctx, OSG_E_UNSUPPORTED, "keyframe database: scoring type %d (only L1)", scoring);
    osg_kfdb *db = new osg_kfdb;
    db->device = ctx->device;
    db->voc_words = nw;
    *out = db;
    return OSG_OK;
}

int osg_kfdb_destroy(osg_kfdb *db)
{
    if (!db) return OSG_E_INVALID;
    (void)hipFree(db->d_word);
    (void)hipFree(db->d_value);
    (void)hipFree(db->d_off);
    (void)hipFree(db->d_len);
    (void)hipFree(db->d_alive);
    for (int k = 0; k < 2; k++) {
        (void)hipFree(db->d_q[k]);
        (void)hipFree(db->d_w[k]);
        (void)hipFree(db->d_s[k]);
    }
    delete db;
    return OSG_OK;
}

int osg_kfdb_size(osg_kfdb *db, int32_t *out)
{
    if (!db || !out) return OSG_E_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    *out = db->n_live;
    return OSG_OK;
}

int osg_kfdb_add(osg_ctx *ctx, osg_kfdb *db, int32_t n_words, const int32_t *word, const double *value, int32_t map_id,
                 const osg_kfdb_state *initial_state, int32_t *entry)
{
    if (!ctx || !db) return OSG_E_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    OSG_RC(same_device(ctx, db));
    OSG_REQUIRE(ctx, entry, "null argument");
    OSG_RC(check_bow(ctx, db, n_words, word, value));
    OSG_REQUIRE(ctx, db->slot_of_entry.size() < (size_t)INT32_MAX, "entry ids exhausted");
    OSG_RC(reserve(ctx, db, n_words));
    const size_t o_v = 256, o_w = o_v + pad256(8 * (size_t)n_words), total = o_w + pad256(4 * (size_t)n_words);
    char *pin = (char *)osg_pinned(ctx, total);
    if (!pin) return osg_set_error(ctx, OSG_E_NOMEM, "pinned alloc failed");
    OSG_RC(osg_idle(ctx));
    osg_kfdb_state st;
    std::memset(&st, 0, sizeof st);
    if (initial_state) st = *initial_state;
    std::memcpy(pin, &st, sizeof st);
    if (n_words) {
        std::memcpy(pin + o_v, value, 8 * (size_t)n_words);
        std::memcpy(pin + o_w, word, 4 * (size_t)n_words);
    }
    const int32_t slot = db->nslots();
    const int blocks = std::max(1, std::min((n_words + 255) / 256, 64));
    hipLaunchKernelGGL(k_kfdb_add, dim3(blocks), dim3(256), 0, ctx->stream, (const osg_kfdb_state *)pin,
                       (const double *)(pin + o_v), (const int32_t *)(pin + o_w), n_words, slot, db->pool_used,
                       db->d_word, db->d_value, db->d_off, db->d_len, db->d_alive, db->d_q[0], db->d_w[0], db->d_s[0],
                       db->d_q[1], db->d_w[1], db->d_s[1]);
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_RC(osg_wait(ctx));
    const int32_t e = (int32_t)db->slot_of_entry.size();
    db->slot_of_entry.push_back(slot);
    db->entry_of_slot.push_back(e);
    db->map_of_slot.push_back(map_id);
    db->len_of_slot.push_back(n_words);
    db->alive.push_back(1);
    db->n_live++;
    db->pool_used += n_words;
    *entry = e;
    return OSG_OK;
}

int osg_kfdb_erase(osg_ctx *ctx, osg_kfdb *db, int32_t entry)
{
    if (!ctx || !db) return OSG_E_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    OSG_RC(same_device(ctx, db));
    OSG_REQUIRE(ctx, entry >= 0 && entry < (int32_t)db->slot_of_entry.size() && db->slot_of_entry[entry] >= 0,
                "entry %d is not in the database", entry);
    const int32_t slot = db->slot_of_entry[entry];
    OSG_HIP_CHECK(ctx, hipMemsetAsync(db->d_alive + slot, 0, 4, ctx->stream));
    OSG_RC(osg_wait(ctx));
    db->slot_of_entry[entry] = -1;
    db->alive[slot] = 0;
    db->n_live--;
    if (db->n_live == 0) clear_locked(db);  // nothing alive: the storage starts over
    return OSG_OK;
}

int osg_kfdb_clear(osg_ctx *ctx, osg_kfdb *db)
{
    if (!ctx || !db) return OSG_E_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    OSG_RC(same_device(ctx, db));
    clear_locked(db);
    return OSG_OK;
}

int osg_kfdb_clear_map(osg_ctx *ctx, osg_kfdb *db, int32_t map_id)
{
    if (!ctx || !db) return OSG_E_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    OSG_RC(same_device(ctx, db));
    const int32_t ns = db->nslots();
    bool any = false;
    for (int32_t s = 0; s < ns; s++) any = any || (db->alive[s] && db->map_of_slot[s] == map_id);
    if (!any) return OSG_OK;
    int32_t *pin = (int32_t *)osg_pinned(ctx, 4 * (size_t)ns);
    if (!pin) return osg_set_error(ctx, OSG_E_NOMEM, "pinned alloc failed");
    OSG_RC(osg_idle(ctx));
    for (int32_t s = 0; s < ns; s++) pin[s] = db->alive[s] && db->map_of_slot[s] != map_id;
    OSG_RC(osg_upload(ctx, db->d_alive, pin, 4 * (size_t)ns));
    OSG_RC(osg_wait(ctx));
    for (int32_t s = 0; s < ns; s++)
        if (db->alive[s] && db->map_of_slot[s] == map_id) {
            db->alive[s] = 0;
            db->slot_of_entry[db->entry_of_slot[s]] = -1;
            db->n_live--;
        }
    if (db->n_live == 0) clear_locked(db);
    return OSG_OK;
}

int osg_kfdb_state_get(osg_ctx *ctx, osg_kfdb *db, int32_t which, int32_t n, const int32_t *entry, int64_t *query,
                       int32_t *words, float *score)
{
    return state_io(ctx, db, which, n, entry, query, words, score, false);
}

int osg_kfdb_state_set(osg_ctx *ctx, osg_kfdb *db, int32_t which, int32_t n, const int32_t *entry, const int64_t *query,
                       const int32_t *words, const float *score)
{
    return state_io(ctx, db, which, n, entry, const_cast<int64_t *>(query), const_cast<int32_t *>(words),
                    const_cast<float *>(score), true);
}

int osg_kfdb_query(osg_ctx *ctx, osg_kfdb *db, int32_t which, int64_t query_id, int32_t n_words, const int32_t *word,
                   const double *value, int32_t n_connected, const int32_t *connected_entries, osg_kfdb_query_out *out)
{
    if (!ctx || !db) return OSG_E_INVALID;
    std::lock_guard<std::mutex> lock(db->mu);
    OSG_RC(same_device(ctx, db));
    OSG_REQUIRE(ctx, out, "null argument");
    OSG_REQUIRE(ctx, which == OSG_KFDB_PLACE || which == OSG_KFDB_RELOC, "detector %d", which);
    OSG_RC(check_bow(ctx, db, n_words, word, value));
    if (which == OSG_KFDB_RELOC) n_connected = 0;
    OSG_REQUIRE(ctx, n_connected >= 0 && (n_connected == 0 || connected_entries), "connected entries");
    out->n_sharing = out->max_common_words = out->min_common_words = out->n_scored = 0;
    OSG_REQUIRE(ctx, out->capacity >= db->n_live && (db->n_live == 0 || (out->entry && out->words && out->score &&
                                                                         out->score_f64)),
                "output arrays hold %d, the database %d entries", out->capacity, db->n_live);
    // GetConnectedKeyFrames as ascending slots (erased entries have none)
    std::vector<int32_t> conn;
    for (int32_t i = 0; i < n_connected; i++) {
        const int32_t e = connected_entries[i];
        OSG_REQUIRE(ctx, e >= 0 && e < (int32_t)db->slot_of_entry.size(), "connected entry %d was never added", e);
        if (db->slot_of_entry[e] >= 0) conn.push_back(db->slot_of_entry[e]);
    }
    std::sort(conn.begin(), conn.end());
    conn.erase(std::unique(conn.begin(), conn.end()), conn.end());
    const int32_t ns = db->nslots();
    if (n_words == 0 || db->n_live == 0) return OSG_OK;
    const int nc = (int)conn.size();
    const int nwg = (ns + WPB - 1) / WPB;
    // pinned: query values, query words, connected slots | header | scored arrays
    const size_t o_qv = 0, o_qw = pad256(8 * (size_t)n_words), o_cn = o_qw + pad256(4 * (size_t)n_words),
                 in_total = o_cn + pad256(4 * (size_t)std::max(nc, 1));
    const size_t r_s64 = 0, r_slot = pad256(8 * (size_t)ns), r_words = r_slot + pad256(4 * (size_t)ns),
                 r_score = r_words + pad256(4 * (size_t)ns), r_total = r_score + pad256(4 * (size_t)ns);
    char *pin = (char *)osg_pinned(ctx, in_total + 256 + r_total);
    if (!pin) return osg_set_error(ctx, OSG_E_NOMEM, "pinned alloc failed");
    OSG_RC(osg_idle(ctx));
    std::memcpy(pin + o_qv, value, 8 * (size_t)n_words);
    std::memcpy(pin + o_qw, word, 4 * (size_t)n_words);
    if (nc) std::memcpy(pin + o_cn, conn.data(), 4 * (size_t)nc);
    char *din = nullptr, *dwork = nullptr, *dres = nullptr;
    OSG_ALLOC(ctx, din, SLOT_TMP0, in_total);
    // work: listed, first, scored (ns each), wg_max, wg_cnt (nwg each), hdr
    const size_t w_listed = 0, w_first = pad256(4 * (size_t)ns), w_scored = 2 * w_first, w_max = 3 * w_first,
                 w_cnt = w_max + pad256(4 * (size_t)nwg), w_hdr = w_cnt + pad256(4 * (size_t)nwg);
    OSG_ALLOC(ctx, dwork, SLOT_TMP1, w_hdr + 256);
    OSG_ALLOC(ctx, dres, SLOT_TMP2, r_total);
    OSG_RC(osg_upload(ctx, din, pin, in_total));
    hipEvent_t *ev = osg_ctx_events(ctx);
    if (!ev) return osg_set_error(ctx, OSG_E_HIP, "event create failed");
    OSG_HIP_CHECK(ctx, hipEventRecord(ev[0], ctx->stream));
    const double *d_qv = (const double *)(din + o_qv);
    const int32_t *d_qw = (const int32_t *)(din + o_qw), *d_cn = (const int32_t *)(din + o_cn);
    int32_t *d_listed = (int32_t *)(dwork + w_listed), *d_first = (int32_t *)(dwork + w_first),
            *d_scored = (int32_t *)(dwork + w_scored), *d_max = (int32_t *)(dwork + w_max),
            *d_cnt = (int32_t *)(dwork + w_cnt), *d_hdr = (int32_t *)(dwork + w_hdr);
    const bool staged = n_words <= Q_STAGE;
    auto count = staged ? k_kfdb_count<true> : k_kfdb_count<false>;
    auto score = staged ? k_kfdb_score<true> : k_kfdb_score<false>;
    hipLaunchKernelGGL(count, dim3(nwg), dim3(QT), 0, ctx->stream, ns, db->d_word, db->d_off, db->d_len, db->d_alive,
                       d_qw, n_words, which, query_id, d_cn, nc, db->d_q[which], db->d_w[which], d_listed, d_first,
                       d_max, d_cnt);
    hipLaunchKernelGGL(k_kfdb_threshold, dim3(1), dim3(TT), 0, ctx->stream, ns, nwg, d_max, d_cnt, d_listed, d_hdr,
                       d_scored);
    hipLaunchKernelGGL(score, dim3(nwg), dim3(QT), 0, ctx->stream, d_hdr, d_scored, db->d_word, db->d_value, db->d_off,
                       db->d_len, d_qw, d_qv, n_words, d_first, d_listed, db->d_s[which], (int32_t *)(dres + r_slot),
                       (int32_t *)(dres + r_words), (float *)(dres + r_score), (double *)(dres + r_s64));
    OSG_HIP_CHECK(ctx, hipGetLastError());
    OSG_HIP_CHECK(ctx, hipEventRecord(ev[1], ctx->stream));
    int32_t *p_hdr = (int32_t *)(pin + in_total);
    OSG_RC(osg_download(ctx, p_hdr, d_hdr, 16));
    OSG_RC(osg_wait(ctx));
    float kms = 0.f;
    OSG_HIP_CHECK(ctx, hipEventElapsedTime(&kms, ev[0], ev[1]));
    ctx->last_kernel_ms = kms;
    const int32_t nsc = p_hdr[3];
    if (nsc < 0 || nsc > db->n_live) return osg_set_error(ctx, OSG_E_HIP, "keyframe database: %d scored entries", nsc);
    out->n_sharing = p_hdr[0];
    out->max_common_words = p_hdr[1];
    out->min_common_words = p_hdr[2];
    out->n_scored = nsc;
    if (nsc == 0) return OSG_OK;
    char *pres = pin + in_total + 256;
    OSG_RC(osg_download(ctx, pres + r_s64, dres + r_s64, 8 * (size_t)nsc));
    OSG_RC(osg_download(ctx, pres + r_slot, dres + r_slot, 4 * (size_t)nsc));
    OSG_RC(osg_download(ctx, pres + r_words, dres + r_words, 4 * (size_t)nsc));
    OSG_RC(osg_download(ctx, pres + r_score, dres + r_score, 4 * (size_t)nsc));
    OSG_RC(osg_wait(ctx));
    const int32_t *p_slot = (const int32_t *)(pres + r_slot);
    for (int32_t i = 0; i < nsc; i++) {
        if (p_slot[i] < 0 || p_slot[i] >= ns) return osg_set_error(ctx, OSG_E_HIP, "keyframe database: slot %d", p_slot[i]);
        out->entry[i] = db->entry_of_slot[p_slot[i]];
    }
    std::memcpy(out->words, pres + r_words, 4 * (size_t)nsc);
    std::memcpy(out->score, pres + r_score, 4 * (size_t)nsc);
    std::memcpy(out->score_f64, pres + r_s64, 8 * (size_t)nsc);
    return OSG_OK;
}

int osg_kfdb_select_nbest(int32_t n, const osg_kfdb_kf *cand, const int32_t *n_neigh, const osg_kfdb_kf *neigh,
                          int64_t query_id, int32_t query_map, int32_t n_candidates, int32_t *loop, int32_t *n_loop,
                          int32_t *merge, int32_t *n_merge)
{
    if (n < 0 || (n && (!cand || !n_neigh || !neigh)) || n_candidates < 0 || !n_loop || !n_merge ||
        (n_candidates && (!loop || !merge)))
        return OSG_E_INVALID;
    std::vector<int32_t> l, m;
    osg_kfdb_nbest(n, cand, n_neigh, neigh, query_id, query_map, n_candidates, l, m);
    *n_loop = (int32_t)l.size();
    *n_merge = (int32_t)m.size();
    for (size_t i = 0; i < l.size(); i++) loop[i] = l[i];
    for (size_t i = 0; i < m.size(); i++) merge[i] = m[i];
    return OSG_OK;
}

int osg_kfdb_select_reloc(int32_t n, const osg_kfdb_kf *cand, const int32_t *n_neigh, const osg_kfdb_kf *neigh,
                          int64_t query_id, int32_t map_id, int32_t *out, int32_t *n_out)
{
    if (n < 0 || (n && (!cand || !n_neigh || !neigh || !out)) || !n_out) return OSG_E_INVALID;
    std::vector<int32_t> r;
    osg_kfdb_reloc(n, cand, n_neigh, neigh, query_id, map_id, r);
    *n_out = (int32_t)r.size();
    for (size_t i = 0; i < r.size(); i++) out[i] = r[i];
    return OSG_OK;
}

}  // extern "C"
