// The one gate between the release library and the tuning build (`make tuning`: -DCCT_TUNING, ../cct_hip/tuning/).
// Every diagnostic switch below is read through TUNING and tuning_env(); no other file tests CCT_TUNING.  In a release
// build TUNING is false and tuning_env() is its default, so the compiler drops every read and the library has no switch
// to set: the outputs of several of them are invalid.  Plain C++: a host compiler reads it without the HIP headers.
//
//   option "debug_skip"   api.cpp -> EncArgs::dbg_skip (encode_tiles.hip): mask of encoder phases to skip, outputs then
//                         invalid; a call with the mask set leaves the stream kernel.  Refused by a release build.
//   option "tuning_build" read-only, 1; the key is unknown to a release build (tools/_inputs.py need_tuning_build)
//   CCT_STREAM_DBG        api.cpp -> StreamArgs::dbg (encode_stream.hip): 1 no carry wait, 2 no look-back (results then
//                         invalid), 4 a wrong group guess on purpose (results valid)
//   CCT_STREAM_STAMPS     encode_stream.hip: launches stream_kernel<.., STAMPS = true> with a buffer of shader clocks per
//                         wave, synchronises and prints the phase split.  Allocates and frees inside the launch path.
//   CCT_INF_PROF          inflate_kernels.hip: launches inflate_kernel<G, PROF = true>, synchronises and prints cycles per phase
//   CCT_J2K_STAGES        api_jpeg2000.cpp -> J2kArgs::stages: the encoder stops early (1 convert and transform, 3 and
//                         Tier-1, 7 all); the files are valid at 7 only
//   CCT_J2K_DEC_STAGES    the same for the decoder (1 parse, 3 and Tier-1, 7 and transform, 15 all); rasters valid at 15 only
//   CCT_TRACE             api.cpp: host timings of every encode and decode call on stderr
//
// Apart from these: -DCCT_TREE_PROF (deflate_kernels.hip, tools/debug/tree_prof.sh) stays a flag of its own.  Its stamps
// and its placement records (where and when every tree wave ran: tools/debug/tree_placement.py) are always on once
// compiled and would perturb the DEFLATE timings the switches above are used to take.
#pragma once
#include <stdlib.h>

namespace cct {

#ifdef CCT_TUNING
constexpr bool TUNING = true;
#else
constexpr bool TUNING = false;
#endif

// The integer value of an environment switch, `dflt` when it is unset; a release build never looks.  The launch paths
// keep the result in a static (one read per name); the JPEG 2000 stage masks and CCT_TRACE are read per call, since the
// stage benchmarks change the mask between calls of one process.
inline int tuning_env(const char *name, int dflt)
{
#ifdef CCT_TUNING
	const char *v = getenv(name);
	return v ? atoi(v) : dflt;
#else
	(void)name;
	return dflt;
#endif
}

}  // namespace cct
