// Stand-alone host program over csrc/kfdb_select.h (step 3 of DetectNBestCandidates and of
// DetectRelocalizationCandidates), driven by tests/test_kfdb.py.
//
// stdin, one problem per line, numbers separated by blanks; a KeyFrame is "query score_bits handle map bad
// map_bad" with score_bits the float's bit pattern as an unsigned integer:
//     P n query_id query_map n_candidates  then per scored KeyFrame: KeyFrame, nn, nn neighbour KeyFrames
//     R n frame_id map_id                  the same
// stdout: "L h h .. M h h .." for P, "C h h .." for R.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "kfdb_select.h"

static osg_kfdb_kf read_kf(std::istream &in)
{
    osg_kfdb_kf k;
    std::memset(&k, 0, sizeof k);
    long long q;
    uint32_t bits;
    int handle, map, bad, map_bad;
    in >> q >> bits >> handle >> map >> bad >> map_bad;
    k.query = q;
    std::memcpy(&k.score, &bits, 4);
    k.handle = handle;
    k.map_id = map;
    k.bad = (uint8_t)bad;
    k.map_bad = (uint8_t)map_bad;
    return k;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char kind;
        if (!(in >> kind)) continue;
        int n;
        long long qid;
        int map, ncand = 0;
        in >> n >> qid >> map;
        if (kind == 'P') in >> ncand;
        // exactly-sized arrays: a read past an end is a sanitizer error
        std::vector<osg_kfdb_kf> cand(n), neigh((size_t)n * OSG_KFDB_MAX_NEIGH);
        std::vector<int32_t> nn(n);
        for (int i = 0; i < n; i++) {
            cand[i] = read_kf(in);
            in >> nn[i];
            for (int j = 0; j < nn[i]; j++) neigh[(size_t)i * OSG_KFDB_MAX_NEIGH + j] = read_kf(in);
        }
        if (!in) {
            std::fprintf(stderr, "bad line\n");
            return 2;
        }
        if (kind == 'P') {
            std::vector<int32_t> loop, merge;
            osg_kfdb_nbest(n, cand.data(), nn.data(), neigh.data(), qid, map, ncand, loop, merge);
            std::printf("L");
            for (int32_t h : loop) std::printf(" %d", h);
            std::printf(" M");
            for (int32_t h : merge) std::printf(" %d", h);
            std::printf("\n");
        } else {
            std::vector<int32_t> out;
            osg_kfdb_reloc(n, cand.data(), nn.data(), neigh.data(), qid, map, out);
            std::printf("C");
            for (int32_t h : out) std::printf(" %d", h);
            std::printf("\n");
        }
    }
    return 0;
}
