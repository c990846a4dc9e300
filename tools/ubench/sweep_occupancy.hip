// what the runtime says about resident blocks per CU of the one-CU 4-wave `_wip` sweeps (spdp_sweep_fp.hip), beside their
// static LDS and register figures: hipOccupancyMaxActiveBlocksPerMultiprocessor for each instantiation a C2 / C4 step
// launches, with 0 and with argv[1..] bytes of dynamic LDS (what SPDP_LDS_PAD adds to a launch).  It divides the CU's LDS
// by the block's bytes; what the hardware makes resident is read from SQ_WAVE_CYCLES (profiles/rows2_c2.txt).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -mno-amdgpu-ieee -fno-slp-vectorize \
//         -I spaln_amd/csrc -o tools/ubench/sweep_occupancy tools/ubench/sweep_occupancy.hip
#include "../../spaln_amd/csrc/spdp_sweep_fp.hip"
#include <cstdio>

template <class K> static void report(const char* name, K kern, int argc, char** argv)
{
    hipFuncAttributes at;
    if (hipFuncGetAttributes(&at, reinterpret_cast<const void*>(kern)) != hipSuccess) { printf("%s: no attributes\n", name); return; }
    printf("%-40s VGPRs %3d  static LDS %6zu B ", name, at.numRegs, at.sharedSizeBytes);
    for (int i = 0; i < argc; ++i) {
        const int dyn = i ? atoi(argv[i]) : 0;
        int nb = -1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, dyn) != hipSuccess) nb = -1;
        printf(" | +%d B: %d blocks / CU", dyn, nb);
    }
    printf("\n");
}

int main(int argc, char** argv)
{
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, 0) != hipSuccess) { printf("no device\n"); return 1; }
    printf("%s: %d CUs, %zu B LDS per CU, %zu B per block\n", pr.gcnArchName, pr.multiProcessorCount, pr.maxSharedMemoryPerMultiProcessor,
           pr.sharedMemPerBlock);
    report("spdp_sweep_fp<FL_UDH,4,false,true>", spdp_sweep_fp<FL_UDH, 4, false, true>, argc, argv);
    report("spdp_sweep_fp<FL_UDH,4,false,true,SIG>", spdp_sweep_fp<FL_UDH, 4, false, true, true>, argc, argv);
    report("spdp_sweep_fp<FL_FORWARD,4,false,true>", spdp_sweep_fp<FL_FORWARD, 4, false, true>, argc, argv);
    report("spdp_sweep_fp<FL_SCORE,4,false,true>", spdp_sweep_fp<FL_SCORE, 4, false, true>, argc, argv);
    return 0;
}
