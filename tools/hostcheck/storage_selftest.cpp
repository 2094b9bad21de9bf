// Stand-alone check of mpm_storage.hpp for a sanitizer: it includes only the header, over the runtime stand-ins of tools/hostcheck/hip/hip_runtime.h
// (malloc / free with a count of live allocations and a "fail the k-th call" switch).  Exit 0 = every case held and nothing is left allocated;
// under -fsanitize=address,undefined a double free, a use after free or a leak aborts instead.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/hostcheck -Iclaymore_amd/csrc
//        -o storage_selftest tools/hostcheck/storage_selftest.cpp
#include "mpm_storage.hpp"
#include <cstdio>
#include <utility>
#include <vector>
using namespace mpm;

static int failures = 0;
#define EXPECT(cond)                                                                           \
	do {                                                                                       \
		if(!(cond)) std::fprintf(stderr, "storage_selftest:%d: %s\n", __LINE__, #cond), ++failures; \
	} while(0)

static long live() {
	return hostcheck_rt().live;
}
static bool all_equal(const int* p, size_t from, size_t to, int v) {
	for(size_t i = from; i < to; ++i)
		if(p[i] != v) return false;
	return true;
}
static void number(int* p, size_t n) {
	for(size_t i = 0; i < n; ++i) p[i] = (int) (i + 1);
}
static bool numbered(const int* p, size_t n) {
	for(size_t i = 0; i < n; ++i)
		if(p[i] != (int) (i + 1)) return false;
	return true;
}

struct TwoBufs {
	int tag = 0;
	DevBuf<int> a;
	DevBuf<float> b;
};

int main() {
	{// alloc(0) is legal and non-null; alloc zero-fills
		DevBuf<int> z;
		EXPECT(z.alloc(0, nullptr) == hipSuccess && z.p != nullptr && z.n == 0 && live() == 1);
		EXPECT(z.p[0] == 0);// (the one element behind n == 0)
		DevBuf<int> b;
		EXPECT(b.alloc(37, nullptr) == hipSuccess && b.n == 37 && all_equal(b, 0, 37, 0));
		int* raw = b;// the implicit conversion, and indexing through it
		EXPECT(raw == b.p && &b[3] == b.p + 3 && b + 5 == b.p + 5);
		// a second alloc replaces the array and frees the old one
		number(b, 37);
		EXPECT(b.alloc(5, nullptr) == hipSuccess && b.n == 5 && all_equal(b, 0, 5, 0) && live() == 2);
	}
	EXPECT(live() == 0);
	{// grow keeps the first n elements and zero-fills the tail; smaller or equal changes nothing
		DevBuf<int> b;
		EXPECT(b.alloc(10, nullptr) == hipSuccess);
		number(b, 10);
		int* before = b.p;
		EXPECT(b.grow(10, nullptr) == hipSuccess && b.p == before && b.n == 10);
		EXPECT(b.grow(3, nullptr) == hipSuccess && b.p == before && b.n == 10 && numbered(b, 10));
		EXPECT(b.grow(16, nullptr) == hipSuccess && b.n == 16 && numbered(b, 10) && all_equal(b, 10, 16, 0) && live() == 1);
		// an empty buffer grows into a zero-filled one; growing from alloc(0) as well
		DevBuf<int> e, z;
		EXPECT(e.grow(4, nullptr) == hipSuccess && e.n == 4 && all_equal(e, 0, 4, 0));
		EXPECT(z.alloc(0, nullptr) == hipSuccess && z.grow(2, nullptr) == hipSuccess && z.n == 2 && all_equal(z, 0, 2, 0));
	}
	EXPECT(live() == 0);
	{// the allocation, the fill, the copy and the synchronisation fail, each in turn: the old array, its contents and n are intact, nothing leaked
		DevBuf<int> b;
		EXPECT(b.alloc(8, nullptr) == hipSuccess);
		number(b, 8);
		int* before = b.p;
		for(HostcheckCall c: {kHcMalloc, kHcMemset, kHcMemcpy, kHcSync}) {
			hostcheck_rt().fail(c, 1);
			EXPECT(b.grow(20, nullptr) != hipSuccess);
			EXPECT(b.p == before && b.n == 8 && numbered(b, 8) && live() == 1);
		}
		for(HostcheckCall c: {kHcMalloc, kHcMemset, kHcSync}) {// ... and a failed alloc keeps what was held
			hostcheck_rt().fail(c, 1);
			EXPECT(b.alloc(20, nullptr) != hipSuccess);
			EXPECT(b.p == before && b.n == 8 && numbered(b, 8) && live() == 1);
		}
		DevBuf<int> e;
		hostcheck_rt().fail(kHcMalloc, 1);
		EXPECT(e.alloc(4, nullptr) == hipErrorOutOfMemory && e.p == nullptr && e.n == 0 && live() == 1);
		EXPECT(b.grow(20, nullptr) == hipSuccess && b.n == 20 && numbered(b, 8) && all_equal(b, 8, 20, 0));// (the switch fires once)
	}
	EXPECT(live() == 0);
	{// a moved-from buffer is empty; move-assignment frees the target's old array exactly once
		DevBuf<int> a, b;
		EXPECT(a.alloc(6, nullptr) == hipSuccess && b.alloc(9, nullptr) == hipSuccess && live() == 2);
		number(a, 6);
		int* pa = a.p;
		DevBuf<int> c(std::move(a));
		EXPECT(a.p == nullptr && a.n == 0 && c.p == pa && c.n == 6 && live() == 2);
		const long frees = hostcheck_rt().frees;
		b = std::move(c);
		EXPECT(hostcheck_rt().frees == frees + 1 && live() == 1 && b.p == pa && b.n == 6 && numbered(b, 6) && c.p == nullptr && c.n == 0);
		DevBuf<int>& self = b;
		b = std::move(self);// (self-assignment keeps the array)
		EXPECT(b.p == pa && b.n == 6 && live() == 1);
	}
	EXPECT(live() == 0);
	{// reset twice is harmless and returns the free's status
		DevBuf<int> b;
		EXPECT(b.alloc(3, nullptr) == hipSuccess);
		EXPECT(b.reset() == hipSuccess && b.p == nullptr && b.n == 0 && live() == 0);
		EXPECT(b.reset() == hipSuccess && live() == 0);
		EXPECT(b.alloc(3, nullptr) == hipSuccess);
		int* held = b.p;
		hostcheck_rt().fail(kHcFree, 1);
		EXPECT(b.reset() == hipErrorInvalidValue && b.p == nullptr && b.n == 0);// the status comes back, the buffer lets go of the array
		EXPECT(b.reset() == hipSuccess);
		EXPECT(hipFree(held) == hipSuccess && live() == 0);// (the stand-in kept it allocated: release it for the leak check)
	}
	{// a std::vector of a struct of DevBufs survives reallocation
		std::vector<TwoBufs> v;
		for(int i = 0; i < 40; ++i) {
			TwoBufs t;
			t.tag = i;
			EXPECT(t.a.alloc(i + 1, nullptr) == hipSuccess && t.b.alloc(2, nullptr) == hipSuccess);
			number(t.a, i + 1);
			v.push_back(std::move(t));
		}
		EXPECT(live() == 80);
		for(int i = 0; i < 40; ++i) EXPECT(v[i].tag == i && v[i].a.n == (size_t) i + 1 && numbered(v[i].a, i + 1) && v[i].b.n == 2);
		v.erase(v.begin() + 3);
		EXPECT(live() == 78 && v[3].tag == 4 && numbered(v[3].a, 5));
	}
	EXPECT(live() == 0);
	{// PinnedBuf: the same for pinned host memory
		PinnedBuf<int> h;
		EXPECT(h.alloc(12) == hipSuccess && h.n == 12 && all_equal(h, 0, 12, 0) && live() == 1);
		PinnedBuf<int> g(std::move(h));
		EXPECT(h.p == nullptr && g.n == 12 && live() == 1);
		hostcheck_rt().fail(kHcHostMalloc, 1);
		EXPECT(g.alloc(4) != hipSuccess && g.n == 12 && live() == 1);
		EXPECT(g.reset() == hipSuccess && g.reset() == hipSuccess && live() == 0);
	}
	EXPECT(live() == 0);
	if(failures) return 1;
	std::printf("storage_selftest ok\n");
	return 0;
}
