// Host stand-in used ONLY by tools/hostcheck (x86 build of mpm_device_math.hpp for quick numerical checks without a GPU).
#pragma once
#include <math.h>
#include <cstdint>
#include <cstring>
#define __device__
#define __forceinline__ inline
#define __global__
#define __restrict__
static inline float __builtin_amdgcn_rcpf(float x) { return 1.0f / x; }
static inline float __builtin_amdgcn_rsqf(float x) { return 1.0f / std::sqrt(x); }
static inline float __builtin_amdgcn_sqrtf(float x) { return std::sqrt(x); }
static inline float __builtin_amdgcn_logf(float x) { return std::log2(x); }
static inline float __builtin_amdgcn_exp2f(float x) { return std::exp2(x); }
static inline bool __all(bool p) { return p; }
static inline bool __any(bool p) { return p; }
static inline float __uint_as_float(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline unsigned __float_as_uint(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

// The few runtime calls of mpm_storage.hpp over malloc / free / memset / memcpy (tools/hostcheck/storage_selftest.cpp): a count of live
// allocations, and a switch that fails the k-th call from now of one kind (k = 1: the next one) with an error of that kind.
#include <cstdlib>
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
typedef struct hostcheck_stream* hipStream_t;
enum HostcheckCall { kHcMalloc, kHcFree, kHcHostMalloc, kHcHostFree, kHcMemset, kHcMemcpy, kHcSync, kHcCalls };
struct HostcheckRuntime {
	long live = 0;// allocations (device and pinned) not freed yet
	long frees = 0;// successful frees so far
	int fail_in[kHcCalls] = {};
	void fail(HostcheckCall c, int k) { fail_in[c] = k; }
	bool failing(HostcheckCall c) { return fail_in[c] > 0 && --fail_in[c] == 0; }
};
inline HostcheckRuntime& hostcheck_rt() {
	static HostcheckRuntime rt;
	return rt;
}
inline hipError_t hostcheck_malloc(HostcheckCall c, void** p, size_t bytes) {
	if(hostcheck_rt().failing(c) || !(*p = std::malloc(bytes))) return hipErrorOutOfMemory;
	std::memset(*p, 0xa5, bytes);// (fresh memory is not zero: the zero-fill under test has to do it)
	++hostcheck_rt().live;
	return hipSuccess;
}
inline hipError_t hostcheck_free(HostcheckCall c, void* p) {
	if(hostcheck_rt().failing(c)) return hipErrorInvalidValue;// (the memory stays allocated, as the caller must assume)
	if(p) std::free(p), --hostcheck_rt().live, ++hostcheck_rt().frees;
	return hipSuccess;
}
inline hipError_t hipMalloc(void** p, size_t bytes) { return hostcheck_malloc(kHcMalloc, p, bytes); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned = 0) { return hostcheck_malloc(kHcHostMalloc, p, bytes); }
inline hipError_t hipFree(void* p) { return hostcheck_free(kHcFree, p); }
inline hipError_t hipHostFree(void* p) { return hostcheck_free(kHcHostFree, p); }
inline hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) {
	if(hostcheck_rt().failing(kHcMemset)) return hipErrorInvalidValue;
	std::memset(p, v, bytes);
	return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t bytes, hipMemcpyKind, hipStream_t) {
	if(hostcheck_rt().failing(kHcMemcpy)) return hipErrorInvalidValue;
	std::memcpy(d, s, bytes);
	return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) { return hostcheck_rt().failing(kHcSync) ? hipErrorUnknown : hipSuccess; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "error"; }
