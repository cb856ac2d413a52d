// host_device.h -- ORBFE_HD marks a function that the kernels and plain host C++ share; ORBFE_UNROLL asks the device compiler to
// unroll the loop that follows (so that arrays indexed by its counter stay in registers) and is nothing to a host compiler.
#pragma once
#if defined(__HIPCC__)
#define ORBFE_HD __host__ __device__
#define ORBFE_UNROLL _Pragma("unroll")
#else
#define ORBFE_HD
#define ORBFE_UNROLL
#endif
