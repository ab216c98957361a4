// The 256x256x64 tile with the 8-phase main loop (igemm_kernel.h, SCHED == 1): same tile id 9, chosen per site class by launch_tile.
#include "igemm_kernel.h"

namespace bs {
int igemm_launch_tile9s8_bf16_cm1(const IgemmParams& p, bool conv, hipStream_t st) { return launch_cm<bf16, 256, 256, 2, 4, 64, 2, false, 1, 1>(p, conv, st); }
}  // namespace bs
