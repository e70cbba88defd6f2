// What the runtime gives the Tier-1 decode kernel of csrc/jpeg2000_decode_kernels.hip: resident workgroups (= waves, one wave a
// code-block) per CU for the LDS of every code-block size, next to the compiler's registers and scratch.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/debug/j2k_dec_occupancy.cpp -o tools/debug/j2k_dec_occupancy && tools/debug/j2k_dec_occupancy
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../2023-compact-image-compression_amd/csrc/jpeg2000_decode_kernels.hip"

int main()
{
	hipFuncAttributes at{};
	if (hipFuncGetAttributes(&at, (const void *)cct::j2k_dec_tier1_kernel) != hipSuccess) { printf("no device\n"); return 1; }
	printf("j2k_dec_tier1_kernel: %d VGPRs, %zu B scratch, %zu B static LDS\n", at.numRegs, at.localSizeBytes, at.sharedSizeBytes);
	const unsigned sizes[][2] = {{6, 6}, {5, 5}, {4, 6}, {4, 4}, {3, 3}, {2, 2}};
	for (auto &s : sizes) {
		int n = 0;
		const size_t lds = cct::j2k_dec_lds_bytes(s[0], s[1]);
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, cct::j2k_dec_tier1_kernel, 64, lds) != hipSuccess) return 1;
		printf("%2u x %2u: %6zu B of LDS, %d waves a CU\n", 1u << s[0], 1u << s[1], lds, n);
	}
	return 0;
}
