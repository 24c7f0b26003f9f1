// ransac_draw.h -- how the RANSAC classes (Sim3Solver.cc, PnPsolver.cc) draw a minimal set: DUtils::Random::RandomInt's arithmetic on the
// C library's rand() and the reference's take-and-swap over the list of available indices.  One definition for both.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace ORB_SLAM2 {

// DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp): the arithmetic on rand()
inline int RansacRandomInt(int min, int max) {
    int d = max - min + 1;
    return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}

// `vAvailableIndices = mvAllIndices;` then k times: `randi = RandomInt(0, size-1); idx = vAvailableIndices[randi]; ...;
// vAvailableIndices[randi] = vAvailableIndices.back(); vAvailableIndices.pop_back();` -- the drawn indices are appended to `out`.
// mvAllIndices is 0 .. N-1 in both classes.
inline void RansacDrawSet(std::vector<size_t>& vAvailableIndices, int N, int k, std::vector<int32_t>& out) {
    vAvailableIndices.resize((size_t)N);
    for (int i = 0; i < N; ++i) vAvailableIndices[i] = i;
    for (short i = 0; i < k; ++i) {
        int randi = RansacRandomInt(0, vAvailableIndices.size() - 1);
        int idx = vAvailableIndices[randi];
        out.push_back(idx);
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
    }
}

}  // namespace ORB_SLAM2
