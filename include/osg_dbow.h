/* osg_dbow.h — DBoW2 vocabulary transform on gfx950.
 *
 * Replaces TemplatedVocabulary<FORB::TDescriptor, FORB>::transform(features, BowVector&,
 * FeatureVector&, levelsup) (ref:Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1126-1192, descent
 * :1214-1256) as called by Frame::ComputeBoW (ref:src/Frame.cc:995-1010, levelsup = 4) and
 * KeyFrame::ComputeBoW.  The FeatureVector comes out as the CSR osg_featvec that
 * osg_search_by_bow_* consume.  No CPU fallback. */
#ifndef OSG_DBOW_H
#define OSG_DBOW_H
#include <stdint.h>

#include "osg.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { OSG_W_TF_IDF = 0, OSG_W_TF = 1, OSG_W_IDF = 2, OSG_W_BINARY = 3 };          /* DBoW2 WeightingType */
enum { OSG_S_L1 = 0, OSG_S_L2 = 1, OSG_S_CHI2 = 2, OSG_S_KL = 3, OSG_S_BHATT = 4, OSG_S_DOT = 5 }; /* ScoringType */

/* A vocabulary as TemplatedVocabulary::loadFromTextFile leaves it in memory
 * (ref:Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1334-1415): node 0 is the root; nodes 1..n-1
 * in file order, each with its parent, leaf flag, 32-byte descriptor and weight.  A node's children
 * are the nodes naming it as parent, in id order; leaves get word ids 0, 1, ... in id order. */
typedef struct osg_vocabulary_desc {
    int32_t k, L;                 /* branching factor, depth levels */
    int32_t scoring, weighting;   /* OSG_S_*, OSG_W_* */
    int32_t n_nodes;              /* including the root */
    const int32_t *parent;        /* n_nodes (parent[0] unused) */
    const uint8_t *is_leaf;       /* n_nodes */
    const uint8_t *desc;          /* n_nodes x 32 (the root's unused) */
    const double *weight;         /* n_nodes */
} osg_vocabulary_desc;

/* BowVector (std::map<WordId, WordValue>) as ascending arrays, and FeatureVector
 * (std::map<NodeId, vector<unsigned>>) as CSR.  Capacities: n_features entries each, node_start
 * n_features + 1. */
typedef struct osg_bow_out {
    int32_t n_words;              /* out */
    int32_t *word;
    double *value;
    int32_t n_nodes;              /* out */
    uint32_t *node_id;
    int32_t *node_start;
    int32_t *feat;
} osg_bow_out;

typedef struct osg_vocabulary osg_vocabulary;

/* Upload a vocabulary to the context's device (breadth-first renumbered so that a node's children
 * are consecutive).  k <= 32. */
int osg_vocabulary_create(osg_ctx *ctx, const osg_vocabulary_desc *v, osg_vocabulary **out);
/* Parse a DBoW2 text vocabulary (ORBvoc.txt format) and upload it. */
int osg_vocabulary_load_text(osg_ctx *ctx, const char *path, osg_vocabulary **out);
int osg_vocabulary_destroy(osg_vocabulary *voc);
/* Sizes of a loaded vocabulary: out4 = {k, L, n_nodes, n_words}. */
int osg_vocabulary_info(const osg_vocabulary *voc, int32_t *out4);

/* transform(features, BowVector, FeatureVector, levelsup) of one descriptor set (n x 32 bytes, the
 * rows of Frame::mDescriptors in order). */
int osg_vocabulary_transform(osg_ctx *ctx, const osg_vocabulary *voc, const uint8_t *desc, int32_t n,
                             int32_t levelsup, osg_bow_out *out);
/* B descriptor sets in one launch: set b has n[b] rows starting at row sum(n[0..b)) of desc;
 * out[b] as above. */
int osg_vocabulary_transform_batch(osg_ctx *ctx, const osg_vocabulary *voc, const uint8_t *desc,
                                   const int32_t *n, int32_t B, int32_t levelsup, osg_bow_out *out);

/* ---- KeyFrameDatabase: BoW place-recognition candidates -------------------------
 *
 * Steps 1 and 2 of KeyFrameDatabase::DetectNBestCandidates (ref:src/KeyFrameDatabase.cc:669-880) and
 * DetectRelocalizationCandidates (:920-1031) on the device: every entry's sorted word list is
 * intersected with the query's, the per-KeyFrame fields mnPlaceRecognitionQuery / Words / Score
 * (mnRelocQuery / Words / Score) are updated as the reference's walk over the inverted file leaves
 * them, and the entries with more than minCommonWords common words are scored (L1) and returned in
 * the order of the reference's lKFsSharingWords.  The covisibility groups, the sort and the choice of
 * candidates work on the caller's KeyFrames: the select calls below (csrc/kfdb_select.h).
 *
 * A database owns a mutex (the reference's mMutex): every call locks it, runs on the calling context's
 * stream and has synchronised before it returns.  Contexts that share a database share its device. */
enum { OSG_KFDB_PLACE = 0, OSG_KFDB_RELOC = 1 };

/* The six per-KeyFrame fields (all 0 on a fresh KeyFrame). */
typedef struct osg_kfdb_state {
    int64_t place_query;          /* mnPlaceRecognitionQuery (long unsigned in the reference) */
    int64_t reloc_query;          /* mnRelocQuery */
    int32_t place_words;          /* mnPlaceRecognitionWords */
    int32_t reloc_words;          /* mnRelocWords */
    float place_score;            /* mPlaceRecognitionScore */
    float reloc_score;            /* mRelocScore */
} osg_kfdb_state;

/* Result of one query.  The arrays hold `capacity` elements each (in), at least the database's size. */
typedef struct osg_kfdb_query_out {
    int32_t n_sharing;            /* out: length of lKFsSharingWords */
    int32_t max_common_words;     /* out */
    int32_t min_common_words;     /* out: int(max_common_words * 0.8f) */
    int32_t n_scored;             /* out: entries with words > min_common_words */
    int32_t capacity;             /* in */
    int32_t *entry;               /* out, n_scored, in the reference's list order */
    int32_t *words;
    float *score;                 /* si */
    double *score_f64;            /* the double si was converted from */
} osg_kfdb_query_out;

typedef struct osg_kfdb osg_kfdb;

/* A database for BowVectors of `voc` (its word count bounds the word ids; its scoring type must be
 * OSG_S_L1, else OSG_E_UNSUPPORTED). */
int osg_kfdb_create(osg_ctx *ctx, const osg_vocabulary *voc, osg_kfdb **out);
int osg_kfdb_destroy(osg_kfdb *db);
/* number of entries (added and not erased) */
int osg_kfdb_size(osg_kfdb *db, int32_t *out);

/* add(pKF): a BowVector as ascending word ids with their values.  *entry is the new entry's id: ids
 * grow by one per add and are never reused, so the id is the position in the add sequence.
 * initial_state: the fields the KeyFrame carries (NULL: zeros).  Words that are not strictly ascending
 * or not below the vocabulary's word count: OSG_E_INVALID. */
int osg_kfdb_add(osg_ctx *ctx, osg_kfdb *db, int32_t n_words, const int32_t *word, const double *value,
                 int32_t map_id, const osg_kfdb_state *initial_state, int32_t *entry);
/* erase(pKF); an id that is not in the database: OSG_E_INVALID */
int osg_kfdb_erase(osg_ctx *ctx, osg_kfdb *db, int32_t entry);
int osg_kfdb_clear(osg_ctx *ctx, osg_kfdb *db);
/* clearMap(pMap): erases every entry added with this map_id */
int osg_kfdb_clear_map(osg_ctx *ctx, osg_kfdb *db, int32_t map_id);

/* The fields of detector `which` of n entries (each in the database): query, words, score arrays of n. */
int osg_kfdb_state_get(osg_ctx *ctx, osg_kfdb *db, int32_t which, int32_t n, const int32_t *entry,
                       int64_t *query, int32_t *words, float *score);
int osg_kfdb_state_set(osg_ctx *ctx, osg_kfdb *db, int32_t which, int32_t n, const int32_t *entry,
                       const int64_t *query, const int32_t *words, const float *score);

/* Steps 1 and 2 of detector `which` for the BowVector (word, value) of a KeyFrame / Frame with id
 * query_id.  connected_entries (OSG_KFDB_PLACE only): GetConnectedKeyFrames as entry ids, each one
 * returned by an earlier add; erased ones are ignored.  An empty query, an empty database or no shared
 * word: zeros in `out`, no state changed. */
int osg_kfdb_query(osg_ctx *ctx, osg_kfdb *db, int32_t which, int64_t query_id, int32_t n_words,
                   const int32_t *word, const double *value, int32_t n_connected,
                   const int32_t *connected_entries, osg_kfdb_query_out *out);

/* A KeyFrame as the selection sees it: the detector's query and score fields after the query, the
 * caller's handle, its map and the isBad() flags of the KeyFrame and of its map. */
typedef struct osg_kfdb_kf {
    int64_t query;
    float score;
    int32_t handle;
    int32_t map_id;
    uint8_t bad, map_bad, pad[2];
} osg_kfdb_kf;
enum { OSG_KFDB_MAX_NEIGH = 10 };

/* Step 3 of DetectNBestCandidates on host arrays (no context, no device): cand[i] the scored entries in
 * list order (score = si), neigh[OSG_KFDB_MAX_NEIGH * i + j], j < n_neigh[i], their
 * GetBestCovisibilityKeyFrames(10).  loop / merge hold n_candidates handles each.  A bad best KeyFrame is
 * skipped (ref:src/KeyFrameDatabase.cc:854 does not advance there). */
int osg_kfdb_select_nbest(int32_t n, const osg_kfdb_kf *cand, const int32_t *n_neigh, const osg_kfdb_kf *neigh,
                          int64_t query_id, int32_t query_map, int32_t n_candidates, int32_t *loop,
                          int32_t *n_loop, int32_t *merge, int32_t *n_merge);
/* The same for DetectRelocalizationCandidates: groups above 0.75f x the best group's score, in list
 * order, of map map_id.  out holds n handles. */
int osg_kfdb_select_reloc(int32_t n, const osg_kfdb_kf *cand, const int32_t *n_neigh, const osg_kfdb_kf *neigh,
                          int64_t query_id, int32_t map_id, int32_t *out, int32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* OSG_DBOW_H */
