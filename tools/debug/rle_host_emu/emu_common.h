// What every emulator's one translation unit needs beside the shim (hip/hip_runtime.h): the shim's thread-local indices and
// block context, defined here because each emulator is a single translation unit, and the helpers of the drivers' file protocol.
#pragma once
#include "hip/hip_runtime.h"
#include <fstream>
#include <iterator>
thread_local dim3 threadIdx, blockIdx, blockDim;
BlockCtx *g_blk;
static inline std::vector<uint8_t> rd(const char *p) { std::ifstream f(p, std::ios::binary); return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), {}); }
// a device buffer is followed by GUARD bytes of 0xEE that must come back untouched
constexpr size_t GUARD = 256;
static inline bool guard_ok(const std::vector<uint8_t> &v, size_t used) { for (size_t k = used; k < v.size(); k++) if (v[k] != 0xEE) return false; return true; }
