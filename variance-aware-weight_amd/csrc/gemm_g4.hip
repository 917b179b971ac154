// The four-wave engine of the bf16 grouped weight gradient (gemm_g4_kernel.h): its one instantiation and its launcher.
#include "gemm_g4_kernel.h"

void vaw_g4_launch_group(int nk, int grid, const EpiDev& e, const P8Prob* probs_dev, const P8Group& grp, hipStream_t s) {
    g4_launch_group(nk, grid, e, probs_dev, grp, s);
}
