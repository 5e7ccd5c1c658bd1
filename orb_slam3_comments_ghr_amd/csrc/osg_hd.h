// osg_hd.h — the qualifier and the loop pragmas of the headers that compile both for the device (hipcc) and as
// plain host C++ (g++ -Wall -Werror: the host test programs, the adapter).
//   OSG_HD        __host__ __device__ under hipcc, nothing otherwise
//   OSG_UNROLL    #pragma unroll under hipcc, nothing otherwise (g++ rejects a pragma it does not know)
//   OSG_UNROLL1   #pragma unroll 1, likewise
#pragma once

#ifdef __HIPCC__
#define OSG_HD __host__ __device__
#define OSG_UNROLL _Pragma("unroll")
#define OSG_UNROLL1 _Pragma("unroll 1")
#else
#define OSG_HD
#define OSG_UNROLL
#define OSG_UNROLL1
#endif
// OSG_HD inline, inlined at every device call site: for the helpers whose array arguments must stay in registers
#ifdef __HIPCC__
#define OSG_HD_FORCEINLINE __host__ __device__ __forceinline__
#else
#define OSG_HD_FORCEINLINE inline
#endif
