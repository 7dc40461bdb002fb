// tm.cpp -- host half of the TM-score path: the per-task scalars that need pow() (parameter_set4search, F/lib/tmalign/TMalign.cpp:25-47, and the d0 of
// standard_TMscore, :1371-1378) and the final scalings (:1423, :622, F/src/commons/TMaligner.cpp:102), computed with this machine's C library as the
// reference computes them.  The searches themselves are k_tm.hpp.  Built like every host object: no -ffast-math; the expressions below hold no
// multiply-add pair a compiler could contract into a different value (each product feeds a cast, a division or a comparison), and the volatile
// temporaries keep the float steps in float.
#include "hostlib.h"

#include <cmath>

extern "C" {

void fshost_tm_params(int normLen, float out[4]) {
    const float Lnorm = (float) normLen;
    volatile float d0;
    if (Lnorm <= 19) d0 = 0.168;
    else { volatile double p = pow(Lnorm * 1.0 - 15, 1.0 / 3); volatile double m = 1.24 * p; d0 = (float) (m - 1.8); }
    volatile float d0min = (float) ((double) d0 + 0.8);
    float d0Search = d0min;
    if (d0Search > 8) d0Search = 8;
    if (d0Search < 4.5) d0Search = 4.5;
    volatile double p8 = pow(Lnorm * 1.0, 0.3);
    volatile double m8 = 1.5 * p8;
    out[0] = (float) (m8 + 3.5);
    volatile float d0Std;
    if (Lnorm > 21) { volatile double p = pow(Lnorm * 1.0 - 15, 1.0 / 3); volatile double m = 1.24 * p; d0Std = (float) (m - 1.8); }
    else d0Std = 0.5f;
    if (d0Std < 0.5f) d0Std = 0.5f;
    out[1] = d0Std;
    out[2] = d0min;
    out[3] = d0Search;
}

double fshost_tm_finish(int nPairs, float s1, float s2, int normLen) {
    const float Lnorm = (float) normLen;
    volatile double a1 = (double) s1 * nPairs;
    volatile double a = a1 / (1.0 * Lnorm);                       // standard_TMscore, in double
    volatile float b1 = s2 * (float) nPairs;
    volatile float b2 = b1 / (float) (int) Lnorm;                 // detailed_search_standard, in float (its Lnorm went through an int)
    const double b = (double) b2;
    return (b < a) ? a : b;                                       // std::max(TM, TMalnScore)
}

// The exact mode (computeExactTMscore, TMaligner.cpp:107-202): score_d8 from parameter_set4search(normLen, normLen), Lnorm / d0 / d0_search from
// parameter_set4final((float) normLen) -- the four floats of a fsgpu_tm_task in that order, Lnorm in the d0Std field.
void fshost_tm_exact_params(int normLen, float out[4]) {
    const float Lnorm = (float) normLen;
    volatile double p8 = pow(Lnorm * 1.0, 0.3);
    volatile double m8 = 1.5 * p8;
    out[0] = (float) (m8 + 3.5);
    out[1] = Lnorm;
    volatile float d0;
    if (Lnorm <= 21) d0 = 0.5f;
    else { volatile double p = pow(Lnorm * 1.0 - 15, 1.0 / 3); volatile double m = 1.24 * p; d0 = (float) (m - 1.8); }
    if (d0 < 0.5f) d0 = 0.5f;
    out[2] = d0;
    float d0Search = d0;
    if (d0Search > 8) d0Search = 8;
    if (d0Search < 4.5) d0Search = 4.5;
    out[3] = d0Search;
}

// TM = (double) score_max; rmsd0 = sqrt(rmsd0 / n_ali8): a float divided by an int, the root taken of that float and stored in a float again
double fshost_tm_exact_finish(int nPairs, float score, float rawRms, float *rmsd) {
    if (rmsd) {
        volatile float q = rawRms / (float) nPairs;
        *rmsd = (float) sqrt((double) q);
    }
    return (double) score;
}

int fshost_tm_normalization(int mode, int alignmentLen, int queryLen, int targetLen) {
    switch (mode) {
        case 0: return alignmentLen;
        case 1: return queryLen;
        case 2: return targetLen;
        default: return 0;
    }
}

} // extern "C"
