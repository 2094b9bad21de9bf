// mpm_storage.hpp — the only place that calls the allocator.  DevBuf<T> owns one device array and knows its element count, PinnedBuf<T>
// is the same for pinned host memory.  Both are move-only, free their array with the scope or the object that holds them, and convert to T*,
// so kernel launches, buf[i], &buf[i], buf + k and hipMemcpy(buf, ...) read as they do with a raw pointer.  Every array is zero from birth:
// what it holds beyond what the kernels wrote does not depend on whether it ever grew.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

namespace mpm {

template<typename T>
struct DevBuf {
	T* p	 = nullptr;
	size_t n = 0;// elements asked for (an empty model is legal: the array behind n == 0 has one element)

	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
	DevBuf& operator=(DevBuf&& o) noexcept {
		if(this != &o) {
			(void) reset();
			p = o.p, n = o.n;
			o.p = nullptr, o.n = 0;
		}
		return *this;
	}
	~DevBuf() { (void) reset(); }
	operator T*() const { return p; }

	// A zero-filled array of max(count, 1) elements in place of whatever was held.  On failure the buffer keeps what it had.
	hipError_t alloc(size_t count, hipStream_t s) {
		T* q		 = nullptr;
		hipError_t e = fresh(&q, count, nullptr, 0, s);
		if(e != hipSuccess) return e;
		(void) reset();
		p = q, n = count;
		return hipSuccess;
	}
	// new_n > n: a zero-filled array of new_n elements that starts with the old contents; the stream is idle when this returns.  On any
	// failure the buffer still owns its old array and its old n.
	hipError_t grow(size_t new_n, hipStream_t s) {
		if(new_n <= n) return hipSuccess;
		T* q		 = nullptr;
		hipError_t e = fresh(&q, new_n, p, n, s);
		if(e != hipSuccess) return e;
		(void) reset();
		p = q, n = new_n;
		return hipSuccess;
	}
	// Frees the array; the buffer is empty afterwards whatever the free reports.
	hipError_t reset() {
		const hipError_t e = p ? hipFree(p) : hipSuccess;
		p = nullptr, n = 0;
		return e;
	}

private:
	static hipError_t fresh(T** out, size_t count, const T* old, size_t old_n, hipStream_t s) {
		const size_t bytes = sizeof(T) * (count ? count : 1);
		T* q			   = nullptr;
		hipError_t e	   = hipMalloc((void**) &q, bytes);
		if(e != hipSuccess) return e;
		if((e = hipMemsetAsync(q, 0, bytes, s)) != hipSuccess || (old && old_n && (e = hipMemcpyAsync(q, old, sizeof(T) * old_n, hipMemcpyDeviceToDevice, s)) != hipSuccess)
		   || (e = hipStreamSynchronize(s)) != hipSuccess) {
			(void) hipFree(q);
			return e;
		}
		*out = q;
		return hipSuccess;
	}
};

// Pinned host memory, zero-filled.
template<typename T>
struct PinnedBuf {
	T* p	 = nullptr;
	size_t n = 0;

	PinnedBuf() = default;
	PinnedBuf(const PinnedBuf&) = delete;
	PinnedBuf& operator=(const PinnedBuf&) = delete;
	PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
	PinnedBuf& operator=(PinnedBuf&& o) noexcept {
		if(this != &o) {
			(void) reset();
			p = o.p, n = o.n;
			o.p = nullptr, o.n = 0;
		}
		return *this;
	}
	~PinnedBuf() { (void) reset(); }
	operator T*() const { return p; }

	hipError_t alloc(size_t count) {
		T* q			   = nullptr;
		const size_t bytes = sizeof(T) * (count ? count : 1);
		const hipError_t e = hipHostMalloc((void**) &q, bytes);
		if(e != hipSuccess) return e;
		memset(q, 0, bytes);
		(void) reset();
		p = q, n = count;
		return hipSuccess;
	}
	hipError_t reset() {
		const hipError_t e = p ? hipHostFree(p) : hipSuccess;
		p = nullptr, n = 0;
		return e;
	}
};

}// namespace mpm
