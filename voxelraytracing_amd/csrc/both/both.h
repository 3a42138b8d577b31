// both.h — the marker of csrc/both/: text that g++ compiles into libvrt_host.so and hipcc into libvrt.so's kernels.  Such a header
// includes only <cstdint>, <cmath>, <cstring>: nothing of HIP, nothing that allocates.  Both libraries are built with
// -ffp-contract=off, the device side with correctly rounded divide and square root and denormals kept (csrc/Makefile): under those
// flags a float expression written once here is the same sequence of correctly rounded binary32 operations on either side.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define VRT_BOTH __host__ __device__ inline
#else
#define VRT_BOTH inline
#endif
