// Stand-in for the CUDA runtime header: the HIP runtime plus the handful of cuda* names the reference
// rasterizer core touches.  Our own text; used only to build oracle/_ref/libgsref.so (oracle/Makefile).
#pragma once
#include <hip/hip_runtime.h>

#define cudaSuccess hipSuccess
#define cudaMemcpy hipMemcpy
#define cudaMemcpyDeviceToHost hipMemcpyDeviceToHost
#define cudaMemset hipMemset
#define cudaDeviceSynchronize hipDeviceSynchronize
#define cudaGetErrorString hipGetErrorString

// CUDA's __trap(); never reached through oracle/ref_cuda/driver.hip (prefiltered is always false).
__device__ inline void __trap() { __builtin_trap(); }
