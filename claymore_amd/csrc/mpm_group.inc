// mpm_group.inc — the MGSP substep loop in C++ (MgspBenchmark::main_loop, Projects/MGSP/mgsp_benchmark.cuh:361-559, with its
// tagging :661-720 and halo exchange :723-776): one group handle per rank, collectives on RCCL directly.
// Included at the end of claymore_hip.hip.
//
// Per substep and rank (everything enqueued, ONE host synchronisation at the end):
//   compute stream: grid update -> G2P2G on the halo particle blocks -> collect the blocks shared with the peers -> [event] ->
//                   G2P2G on the interior blocks -> [wait] -> partition rebuild -> padded key export -> ncclAllGather(keys) ->
//                   overlap marks / send lists / halo split
//   comm stream:    [event] -> ncclGroup{ncclSend, ncclRecv per peer} -> reduce -> [event back]
// (the send / receive is enqueued BEFORE the interior G2P2G: see grp_exchange_halo)
// The exchange is symmetric (a block shared with p is sent to p and received from p), so receive counts equal send counts
// and no count exchange is needed; the grouped send/recv drives all xGMI links of a GPU at once.  The reference does the
// same moves with one worker thread per GPU and pairwise cudaMemcpyPeerAsync (mgsp_benchmark.cuh:309-356, halo_buffer.cuh:54-59).
//
// Two transports behind one interface:
//   * RCCL (mpm_group_create): one rank per process or per thread, one GPU each - the product path;
//   * in-process hub (mpm_group_create_local): all ranks live in one process and may even share a device (several engine
//     contexts on one GPU): device-to-device copies between the ranks' buffers, rendez-vous on a host barrier.  This is
//     what a single-GPU box can run, and what the multi-context tests use; RCCL cannot host two ranks on one device.
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <atomic>
#include <condition_variable>
#include <mutex>

namespace {

// RCCL is loaded on first use: contexts that never form a group do not need the library at all.
struct Rccl {
	void* lib = nullptr;
	ncclResult_t (*GetUniqueId)(ncclUniqueId*)																  = nullptr;
	ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int)											  = nullptr;
	ncclResult_t (*CommDestroy)(ncclComm_t)																	  = nullptr;
	ncclResult_t (*CommAbort)(ncclComm_t)																		  = nullptr;// (optional)
	ncclResult_t (*CommCount)(const ncclComm_t, int*)															  = nullptr;// (optional)
	ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t)				  = nullptr;
	ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)					  = nullptr;
	ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)							  = nullptr;
	ncclResult_t (*GroupStart)()																				  = nullptr;
	ncclResult_t (*GroupEnd)()																					  = nullptr;
	const char* (*GetErrorString)(ncclResult_t)																  = nullptr;
};
Rccl* rccl() {
	static Rccl r;
	static std::once_flag once;
	std::call_once(once, [] {
		// MPM_RCCL_LIBRARY: the collective library to load instead of the system's RCCL (a differently built RCCL; the tests' in-process
		// double of the ncclSend / ncclRecv / ncclAllGather / ncclAllReduce calls, tests/rccl_double/)
		const char* path = getenv("MPM_RCCL_LIBRARY");
		const char* from = nullptr;
		if(path && path[0]) {// (an empty value counts as unset)
			r.lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
			from  = path;
		} else {
			for(const char* name: {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
				r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
				from  = name;
				if(r.lib) break;
			}
		}
		if(getenv("MPM_GROUP_VERBOSE") || (path && path[0])) fprintf(stderr, "claymore_hip: collective library %s%s\n", r.lib ? from : "NOT FOUND", path && path[0] ? " (MPM_RCCL_LIBRARY)" : "");
		if(!r.lib) return;
#define MPM_SYM(field, sym) r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.lib, sym))
		MPM_SYM(GetUniqueId, "ncclGetUniqueId");
		MPM_SYM(CommInitRank, "ncclCommInitRank");
		MPM_SYM(CommDestroy, "ncclCommDestroy");
		MPM_SYM(CommAbort, "ncclCommAbort");
		MPM_SYM(CommCount, "ncclCommCount");
		MPM_SYM(AllGather, "ncclAllGather");
		MPM_SYM(AllReduce, "ncclAllReduce");
		MPM_SYM(Send, "ncclSend");
		MPM_SYM(Recv, "ncclRecv");
		MPM_SYM(GroupStart, "ncclGroupStart");
		MPM_SYM(GroupEnd, "ncclGroupEnd");
		MPM_SYM(GetErrorString, "ncclGetErrorString");
#undef MPM_SYM
		if(!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.AllReduce || !r.Send || !r.Recv || !r.GroupStart || !r.GroupEnd) {
			dlclose(r.lib);
			r.lib = nullptr;
		}
	});
	return r.lib ? &r : nullptr;
}

// rendez-vous of the ranks of one process (in-process transport)
struct LocalHub {
	int world = 0;
	std::mutex m;
	std::condition_variable cv;
	int waiting = 0, generation = 0, refs = 0;
	bool broken = false;
	const void* ptr[32] = {};
	const size_t* offs[32] = {};
	int dev[32]		 = {};// the device each rank's context lives on
	bool peer_direct = false;// PEER-DIRECT transport: the ranks sit on different devices of this process with peer access enabled (or MPM_GROUP_TRANSPORT=peer
							 // asks for its code path on one device): halo blocks and key lists move with hipMemcpyPeerAsync over xGMI, the reference's
							 // own mechanism (cudaMemcpyPeerAsync, Projects/MGSP/halo_buffer.cuh:54-59; peer access: Library/MnSystem/Cuda/Cuda.cu:120-127)
	float scalar[32]	= {};
	hipEvent_t ev_sent[32] = {};// asynchronous exchange: rank r's send buffer is complete / rank r has copied what it receives
	hipEvent_t ev_done[32] = {};
	std::atomic<bool> have_done {false};
	hipEvent_t ev_keys[32] = {};// asynchronous key all-gather: rank r's key list is complete / rank r has copied every list
	hipEvent_t ev_kdone[32] = {};
	std::atomic<bool> have_kdone {false};
	bool wait() {// false if a rank gave up (error elsewhere): nobody may block forever
		std::unique_lock<std::mutex> lk(m);
		if(broken) return false;
		const int gen = generation;
		if(++waiting == world) {
			waiting = 0;
			++generation;
			cv.notify_all();
			return true;
		}
		cv.wait(lk, [&] { return gen != generation || broken; });
		return !broken;
	}
	void abort() {
		std::lock_guard<std::mutex> lk(m);
		broken = true;
		cv.notify_all();
	}
};

}// namespace

struct mpm_group {
	mpm_ctx* ctx = nullptr;
	int rank = 0, world = 1;
	ncclComm_t comm = nullptr;
	LocalHub* hub	= nullptr;
	int pad			= 0;// padded key-list length (rows of 3 ints, row 0 = true count) of the tagging all-gather
	DevBuf<int> d_keys_mine, d_keys_all;// 3 pad ints and world times that (grp_key_buffers): d_keys_all, allocated last, says what padding both hold
	DevBuf<float> d_send, d_recv;// the same number of floats each (grp_halo_capacity): d_recv, allocated last, says how many both hold
	DevBuf<float> d_scalar;
	int send_counts[32] = {};
	size_t offs[33]		= {};
	int n_halo_blocks	= 0;
	double g2p2g_ms_sum = 0;
	long steps			= 0;
	bool early_exchange = false;// see grp_exchange_halo
	bool no_defer		= false;// MPM_GROUP_DEFER=0: mpm_group_run_fixed waits for every substep's read-back at once (A/B, debugging)
	bool overlap_tag	= false;// MPM_GROUP_OVERLAP_TAG=1: the tagging chain of a substep on the comm stream beside the rebuild's last kernel (see grp_substep_tail; off by default)
	bool tight_pad		= false;// MPM_GROUP_PAD_TIGHT=1 (tests): no slack in the key-list padding - every growth truncates, the recovery paths run all the time
	int retags			= 0;// key lists that outgrew their padding inside mpm_group_run_fixed / mpm_group_substep and were tagged again
	bool aborted		= false;// the communicator was aborted after an RCCL error
	int pad_enqueued	= 0;	// the padding the outstanding substep's key lists were exported with
	// the windowed loop waits for the status read-back of substep t AFTER the halo-first G2P2G of substep t + 1 has been enqueued, so its
	// timing events exist twice (index = parity of the substep); a call of one substep times it with the context's own set
	SubstepEvents ev2[2];
	hipEvent_t ev_sent = nullptr, ev_done = nullptr;// in-process transport, asynchronous exchange
	hipEvent_t ev_keys = nullptr, ev_kdone = nullptr;// ... and asynchronous key all-gather
	std::string err;
};

namespace {
int gfail(mpm_group* g, int code, const std::string& msg) {
	g->err = msg;
	if(g->ctx && !msg.empty()) g->ctx->err = msg;
	if(g->hub) g->hub->abort();
	return code;
}
#define GRP_HIP(expr)                                                                                        \
	do {                                                                                                     \
		hipError_t e_ = (expr);                                                                              \
		if(e_ != hipSuccess) return gfail(g, MPM_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
	} while(0)
// a collective that failed leaves the communicator in an undefined state: it is aborted (its outstanding operations are cancelled, the
// destroy at the end cannot block), every later call of this group fails at once
int grp_nccl_fail(mpm_group* g, const char* what, ncclResult_t r) {
	const std::string msg = std::string(what) + ": " + (rccl()->GetErrorString ? rccl()->GetErrorString(r) : "rccl error");
	if(g->comm && rccl()->CommAbort) {
		rccl()->CommAbort(g->comm);
		g->comm = nullptr;
	}
	g->aborted = true;// (also without ncclCommAbort in the loaded library: the communicator's state is undefined, nothing may use it again -
					  //  mpm_group_destroy then leaves it alone, a destroy could block on the operation that failed)
	return gfail(g, MPM_ERR_DEVICE, msg);
}
#define GRP_NCCL(expr)                                       \
	do {                                                     \
		ncclResult_t r_ = (expr);                            \
		if(r_ != ncclSuccess) return grp_nccl_fail(g, #expr, r_); \
	} while(0)
#define GRP_TRY(expr)                                                   \
	do {                                                                \
		int rc_ = (expr);                                               \
		if(rc_) return gfail(g, rc_, g->ctx ? g->ctx->err : ""); \
	} while(0)

// device-to-device copy between two ranks of one process: a peer copy (xGMI, no staging through the host) on the peer-direct transport
hipError_t grp_hub_copy(const mpm_group* g, void* dst, const void* src, int src_rank, size_t bytes, hipStream_t s) {
	const LocalHub* h = g->hub;
	if(h->peer_direct) return hipMemcpyPeerAsync(dst, h->dev[g->rank], src, h->dev[src_rank], bytes, s);
	return hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, s);
}

// ---- the three collectives ------------------------------------------------------------------------------------
int grp_all_gather(mpm_group* g, const int* send, int* recv, size_t ints_per_rank, hipStream_t s) {
	if(g->aborted) return gfail(g, MPM_ERR_DEVICE, "the RCCL communicator was aborted after an error");
	if(g->comm) {
		GRP_NCCL(rccl()->AllGather(send, recv, ints_per_rank, ncclInt32, g->comm, s));
		return MPM_OK;
	}
	LocalHub* h = g->hub;
	if(g->early_exchange && g->ev_keys) {// asynchronous variant: host barriers hand over pointers and events, the GPU waits on events (see grp_exchange)
		GRP_HIP(hipEventRecord(g->ev_keys, s));
		h->ptr[g->rank]		= send;
		h->ev_keys[g->rank] = g->ev_keys;
		if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
		for(int p = 0; p < g->world; ++p) {
			if(p != g->rank) GRP_HIP(hipStreamWaitEvent(s, h->ev_keys[p], 0));
			GRP_HIP(grp_hub_copy(g, recv + (size_t) p * ints_per_rank, h->ptr[p], p, sizeof(int) * ints_per_rank, s));
		}
		GRP_HIP(hipEventRecord(g->ev_kdone, s));
		h->ev_kdone[g->rank] = g->ev_kdone;
		if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
		h->have_kdone = true;
		return MPM_OK;
	}
	GRP_HIP(hipStreamSynchronize(s));
	h->ptr[g->rank] = send;
	if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
	for(int p = 0; p < g->world; ++p) GRP_HIP(grp_hub_copy(g, recv + (size_t) p * ints_per_rank, h->ptr[p], p, sizeof(int) * ints_per_rank, s));
	GRP_HIP(hipStreamSynchronize(s));
	if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
	return MPM_OK;
}
// symmetric all-to-all-v: offs[p]..offs[p+1] (floats) is what goes to AND comes from peer p
int grp_exchange(mpm_group* g, const float* send, float* recv, const size_t* offs, hipStream_t s) {
	if(g->aborted) return gfail(g, MPM_ERR_DEVICE, "the RCCL communicator was aborted after an error");
	if(g->comm) {
		GRP_NCCL(rccl()->GroupStart());
		ncclResult_t bad = ncclSuccess;// (a group that was started is always ended: an open group would swallow every later call of this thread)
		for(int p = 0; p < g->world && bad == ncclSuccess; ++p) {
			const size_t n = offs[p + 1] - offs[p];
			if(p == g->rank || n == 0) continue;
			bad = rccl()->Send(send + offs[p], n, ncclFloat32, p, g->comm, s);
			if(bad == ncclSuccess) bad = rccl()->Recv(recv + offs[p], n, ncclFloat32, p, g->comm, s);
		}
		const ncclResult_t ended = rccl()->GroupEnd();
		GRP_NCCL(bad);
		GRP_NCCL(ended);
		return MPM_OK;
	}
	LocalHub* h = g->hub;
	if(g->early_exchange && g->ev_sent) {
		// Asynchronous variant (what the RCCL transport does, with device-to-device copies in place of ncclSend / ncclRecv): nothing waits
		// on the host for the GPU.  The ranks meet at host barriers only to hand over pointers and events; a rank's copies wait (on the
		// device) for the peer's "send buffer complete" event, and a peer's NEXT collect waits for this rank's "copied" event.
		GRP_HIP(hipEventRecord(g->ev_sent, s));
		h->ptr[g->rank]		= send;
		h->offs[g->rank]	= offs;
		h->ev_sent[g->rank] = g->ev_sent;
		if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
		for(int p = 0; p < g->world; ++p) {
			const size_t n = offs[p + 1] - offs[p];
			if(p == g->rank || n == 0) continue;
			const size_t* po = h->offs[p];
			if(po[g->rank + 1] - po[g->rank] != n) return gfail(g, MPM_ERR_INVALID, "halo exchange is not symmetric");
			GRP_HIP(hipStreamWaitEvent(s, h->ev_sent[p], 0));
			GRP_HIP(grp_hub_copy(g, recv + offs[p], static_cast<const float*>(h->ptr[p]) + po[g->rank], p, sizeof(float) * n, s));
		}
		GRP_HIP(hipEventRecord(g->ev_done, s));
		h->ev_done[g->rank] = g->ev_done;
		if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
		h->have_done = true;
		return MPM_OK;
	}
	GRP_HIP(hipStreamSynchronize(s));
	h->ptr[g->rank]	 = send;
	h->offs[g->rank] = offs;
	if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
	for(int p = 0; p < g->world; ++p) {
		const size_t n = offs[p + 1] - offs[p];
		if(p == g->rank || n == 0) continue;
		const size_t* po = h->offs[p];
		if(po[g->rank + 1] - po[g->rank] != n) return gfail(g, MPM_ERR_INVALID, "halo exchange is not symmetric");
		GRP_HIP(grp_hub_copy(g, recv + offs[p], static_cast<const float*>(h->ptr[p]) + po[g->rank], p, sizeof(float) * n, s));
	}
	GRP_HIP(hipStreamSynchronize(s));
	if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
	return MPM_OK;
}
int grp_all_reduce_max(mpm_group* g, float* v) {
	if(g->aborted) return gfail(g, MPM_ERR_DEVICE, "the RCCL communicator was aborted after an error");
	if(g->comm) {
		hipStream_t s = g->ctx->s_compute;
		GRP_HIP(hipMemcpyAsync(g->d_scalar, v, sizeof(float), hipMemcpyHostToDevice, s));
		GRP_NCCL(rccl()->AllReduce(g->d_scalar, g->d_scalar, 1, ncclFloat32, ncclMax, g->comm, s));
		GRP_HIP(hipMemcpyAsync(v, g->d_scalar, sizeof(float), hipMemcpyDeviceToHost, s));
		GRP_HIP(hipStreamSynchronize(s));
		return MPM_OK;
	}
	LocalHub* h		   = g->hub;
	h->scalar[g->rank] = *v;
	if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
	float m = h->scalar[0];
	for(int p = 1; p < g->world; ++p) m = std::max(m, h->scalar[p]);
	if(!h->wait()) return gfail(g, MPM_ERR_DEVICE, "group aborted");
	*v = m;
	return MPM_OK;
}

int grp_key_buffers(mpm_group* g) {
	if(g->hub && g->hub->have_kdone) {// (asynchronous in-process gather: the peers may still be reading d_keys_mine)
		const bool realloc = g->d_keys_all.n != 3 * (size_t) g->pad * g->world;
		for(int p = 0; p < g->world; ++p)
			if(p != g->rank && g->hub->ev_kdone[p]) {
				if(realloc)
					GRP_HIP(hipEventSynchronize(g->hub->ev_kdone[p]));
				else
					GRP_HIP(hipStreamWaitEvent(g->ctx->s_compute, g->hub->ev_kdone[p], 0));
			}
	}
	if(g->d_keys_all.n == 3 * (size_t) g->pad * g->world) return MPM_OK;
	GRP_HIP(hipStreamSynchronize(g->ctx->s_compute));
	(void) g->d_keys_mine.reset();
	(void) g->d_keys_all.reset();
	GRP_HIP(g->d_keys_mine.alloc(3 * (size_t) g->pad, g->ctx->s_compute));
	GRP_HIP(g->d_keys_all.alloc(3 * (size_t) g->pad * g->world, g->ctx->s_compute));
	return MPM_OK;
}

// Padding of the key lists that travel in the tagging all-gather (row 0 = true count).  A list that outgrows its padding is truncated for
// that one tagging and every rank sees it (same row 0s): the tagging is repeated with the larger length - at once where the host waits at
// the end of the substep, after the substep's two G2P2G passes in the windowed loop (mpm_group_run_fixed).  Both cost a host round trip, so
// the padding grows ahead of time: at 3/4 fill to 3/2 of the longest list (round 4: at 9/10 to 5/4 - a slab a few blocks thick whose face
// crosses a block boundary adds a whole layer of blocks in one substep, +12.5 % at eight blocks).  12 B per row: 3/2 of 12 k blocks are 220 KB.
// `rows` counts row 0 (the {true count, status word} header) everywhere: a list of n keys needs n + 1 rows, n_in = min(count, pad - 1) keys
// fit a padding of `pad` rows, and a padding below 2 rows holds no key at all (mgsp_rebuild_export rejects it): clamped here, not at the call sites.
int grp_pad_for(const mpm_group* g, int rows) {
	return std::max(2, g->tight_pad ? rows : (int) (1.5 * rows) + 64);
}
bool grp_pad_close(const mpm_group* g, int rows, int pad) {
	return g->tight_pad ? rows > pad : rows > 0.75 * pad;
}

// Tagging at set-up, on resume and after a truncation (mgsp_benchmark.cuh:661-720): the substep's chain - key export -> all-gather ->
// marks / send lists / halo split - on the current partition, then one read-back of the halo counts and the row-0 heads.  A list that
// was truncated (some head + 1 > pad) is tagged again with the larger padding.
int grp_tag(mpm_group* g) {
	mpm_ctx* ctx = g->ctx;
	if(g->pad == 0) {// first call: agree on a padded length (every later length is derived from gathered counts)
		float n = (float) ctx->nbc;
		int rc	= grp_all_reduce_max(g, &n);
		if(rc) return rc;
		g->pad = std::max(2, grp_pad_for(g, (int) n + 1));
	}
	GRP_HIP(hipSetDevice(ctx->device));
	GRP_TRY(halo_alloc(ctx));
	for(;;) {
		const int pad = g->pad;// identical on all ranks by construction
		int rc		  = grp_key_buffers(g);
		if(rc) return rc;
		ctx->halo_tagged = false;
		GRP_TRY(halo_export(ctx, ctx->rollid, g->d_keys_mine, pad));
		rc = grp_all_gather(g, g->d_keys_mine, g->d_keys_all, 3 * (size_t) pad, ctx->s_compute);
		if(rc) return rc;
		GRP_TRY(halo_tag(ctx, ctx->rollid, g->d_keys_all, pad, g->world, g->rank, ctx->s_compute));
		GRP_TRY(halo_read_counts(ctx, g->world));
		int need = 0;
		for(int p = 0; p < g->world; ++p) need = std::max(need, ctx->h_peer_rows[p] + 1);
		if(need > pad) {// some rank outgrew the padding: every rank sees it and repeats with the same larger length
			g->pad = grp_pad_for(g, need);
			continue;
		}
		if(grp_pad_close(g, need, pad)) g->pad = grp_pad_for(g, need);// grow ahead of time (takes effect at the next tagging)
		g->n_halo_blocks = ctx->n_halo;
		for(int p = 0; p < 32; ++p) g->send_counts[p] = p == g->rank ? 0 : ctx->send_count[p];
		return MPM_OK;
	}
}

// The halo exchange: collect -> all-to-all-v -> reduce, built from the helpers below in two orders.
// Order matters for overlap.  The interior G2P2G fills every SIMD's register file with single-wave workgroups and refills
// each slot a retiring wave frees at once, so a kernel that becomes ready while it runs - a 256-thread collect, RCCL's
// send / receive workgroups - finds no room until it drains, whatever its stream priority (profiles/r02_mgsp_timeline.txt).
// With early_exchange (RCCL transport) the collect therefore runs on the compute stream right behind the halo-first
// G2P2G, and the grouped send / receive is enqueued on the high-priority comm stream BEFORE the interior G2P2G: both
// become ready at the same event, on an empty GPU, and the transfer runs beside the interior blocks.  (The in-process
// transport synchronises the host inside the exchange, so there the interior launch goes first and the collect runs on the
// comm stream, so that host time spent in the collective does not delay the interior launch: mgsp_benchmark.cuh:449-466, :723-776.)
// The windowed loop (mpm_group_run_fixed) splits the early order in two halves: grp_halo_compute_half, sized from device memory,
// and grp_halo_comm_half, which needs the counts on the host.
size_t grp_halo_offsets(mpm_group* g) {
	g->offs[0] = 0;
	for(int p = 0; p < g->world; ++p) g->offs[p + 1] = g->offs[p] + kHaloRow * (size_t) (p == g->rank ? 0 : g->send_counts[p]);
	return g->offs[g->world];
}
int grp_halo_capacity(mpm_group* g, size_t total) {
	if(total <= g->d_recv.n) return MPM_OK;
	if(g->hub && g->hub->have_done)// (asynchronous in-process exchange: no peer may still be reading the buffer that is about to go)
		for(int p = 0; p < g->world; ++p)
			if(p != g->rank && g->hub->ev_done[p]) GRP_HIP(hipEventSynchronize(g->hub->ev_done[p]));
	GRP_HIP(hipDeviceSynchronize());
	(void) g->d_send.reset();
	(void) g->d_recv.reset();
	const size_t xcap = total + total / 2 + kHaloRow;
	GRP_HIP(g->d_send.alloc(xcap, g->ctx->s_compute));
	GRP_HIP(g->d_recv.alloc(xcap, g->ctx->s_compute));
	return MPM_OK;
}
// asynchronous in-process exchange: the peers may still be reading d_send
int grp_wait_peers_done(mpm_group* g) {
	if(!(g->hub && g->ev_sent && g->hub->have_done)) return MPM_OK;
	for(int p = 0; p < g->world; ++p)
		if(p != g->rank && g->hub->ev_done[p]) {
			GRP_HIP(hipStreamWaitEvent(g->ctx->s_compute, g->hub->ev_done[p], 0));
			GRP_HIP(hipStreamWaitEvent(g->ctx->s_comm, g->hub->ev_done[p], 0));
		}
	return MPM_OK;
}
// every peer's blocks into d_send, in one launch on stream s (sizes from device memory); counts_known: g->send_counts are those of the
// last tagging (otherwise one tagging old: they only size the launch)
int grp_collect(mpm_group* g, int gid, hipStream_t s, bool counts_known = true) {
	int est = 0;
	for(int p = 0; p < g->world; ++p) est = std::max(est, p == g->rank ? 0 : g->send_counts[p]);
	if(g->world > 1 && g->d_send && (est > 0 || !counts_known)) GRP_TRY(halo_collect(g->ctx, s, gid, 0, g->world, g->rank, est, g->d_send, g->d_recv.n));
	return MPM_OK;
}
// the received blocks into grid gid (comm stream); the compute stream waits for them
int grp_reduce(mpm_group* g, int gid) {
	mpm_ctx* ctx = g->ctx;
	bool any	 = false;
	for(int p = 0; p < g->world; ++p) {
		const int c = p == g->rank ? 0 : g->send_counts[p];
		if(!c) continue;
		const float* base = g->d_recv + g->offs[p];
		GRP_TRY(mpm_halo_reduce(ctx, gid, reinterpret_cast<const int*>(base), base + 3 * (size_t) c, c));
		any = true;
	}
	if(!any) GRP_TRY(mpm_halo_reduce(ctx, gid, nullptr, nullptr, 0));// nothing shared: still order the compute stream behind the comm stream
	return MPM_OK;
}
int grp_send_recv(mpm_group* g) {
	return g->world > 1 ? grp_exchange(g, g->d_send, g->d_recv, g->offs, g->ctx->s_comm) : MPM_OK;
}
// interior: the interior G2P2G of this substep is enqueued too (plan.ev.g2p2g_end marks its end)
int grp_exchange_halo(mpm_group* g, const SubstepPlan& plan, int gid, bool interior) {
	mpm_ctx* ctx	 = g->ctx;
	const bool early = g->early_exchange && interior;
	int rc			 = grp_halo_capacity(g, grp_halo_offsets(g));
	if(rc || (rc = grp_wait_peers_done(g))) return rc;
	if(interior && !early) GRP_TRY(g2p2g_interior(ctx, plan));
	if((rc = grp_collect(g, gid, early ? ctx->s_compute : ctx->s_comm))) return rc;
	if(early) {
		GRP_HIP(hipEventRecord(ctx->ev_halo, ctx->s_compute));
		GRP_HIP(hipStreamWaitEvent(ctx->s_comm, ctx->ev_halo, 0));
	}
	if((rc = grp_send_recv(g))) return rc;
	if(early) GRP_TRY(g2p2g_interior(ctx, plan));
	return grp_reduce(g, gid);
}
// Compute half: the collect right behind the halo-first G2P2G, then the interior G2P2G, all on the compute stream - it can be enqueued
// while the read-back of the previous substep's counts is still outstanding.
int grp_halo_compute_half(mpm_group* g, const SubstepPlan& plan, int gid) {
	mpm_ctx* ctx			= g->ctx;
	const bool counts_known = !plan.counts_pending;
	int rc					= counts_known ? grp_halo_capacity(g, grp_halo_offsets(g)) : MPM_OK;// (otherwise the buffer of the last exchange is used: the comm half checks it against the counts)
	if(rc || (rc = grp_wait_peers_done(g)) || (rc = grp_collect(g, gid, ctx->s_compute, counts_known))) return rc;
	GRP_HIP(hipEventRecord(ctx->ev_halo, ctx->s_compute));
	GRP_TRY(g2p2g_interior(ctx, plan));
	return MPM_OK;
}
// Comm half (needs the counts on the host): the grouped send / receive and the reduce on the comm stream, which waits for the collect's
// event; by then the interior launch is running, the transfer goes on beside it.
int grp_halo_comm_half(mpm_group* g, int gid, bool collect_again = false) {
	mpm_ctx* ctx	   = g->ctx;
	const size_t total = grp_halo_offsets(g);
	if(total > g->d_recv.n || collect_again) {// the counts outgrew the buffer the collect ran into (grow it), or the send lists were rebuilt after it ran: collect again (behind the interior launch, this once)
		int rc = grp_halo_capacity(g, total);
		if(rc || (rc = grp_collect(g, gid, ctx->s_compute))) return rc;
		GRP_HIP(hipEventRecord(ctx->ev_halo, ctx->s_compute));
	}
	GRP_HIP(hipStreamWaitEvent(ctx->s_comm, ctx->ev_halo, 0));
	int rc = grp_send_recv(g);
	return rc ? rc : grp_reduce(g, gid);
}

int grp_common_init(mpm_group* g) {
	g->ctx->group_refs++;// (undone by mpm_group_destroy, which every failure below leads to)
	if(g->ctx->body_mask) {// (the handle does not outlive the refusal: the context keeps the message)
		g->ctx->err = "a context with a rigid body (mpm_set_collider_body) cannot join a group: bodies in multi-GPU groups are not computed";
		return gfail(g, MPM_ERR_INVALID, g->ctx->err);
	}
	if(g->ctx->force.count) {
		g->ctx->err = "a context with a force field (mpm_set_force_field) cannot join a group: force fields in multi-GPU groups are not computed";
		return gfail(g, MPM_ERR_INVALID, g->ctx->err);
	}
	if(const char* e = getenv("MPM_GROUP_DEFER")) g->no_defer = e[0] == '0';
	if(const char* e = getenv("MPM_GROUP_PAD_TIGHT")) g->tight_pad = e[0] == '1';
	if(const char* e = getenv("MPM_GROUP_OVERLAP_TAG")) g->overlap_tag = e[0] != '0';
	GRP_HIP(hipSetDevice(g->ctx->device));
	GRP_HIP(g->d_scalar.alloc(1, g->ctx->s_compute));
	for(SubstepEvents& ev: g->ev2)
		for(hipEvent_t* e: {&ev.start, &ev.g2p2g_start, &ev.g2p2g_end, &ev.end}) GRP_HIP(hipEventCreate(e));
	if(g->hub && g->early_exchange) {
		GRP_HIP(hipEventCreateWithFlags(&g->ev_sent, hipEventDisableTiming));
		GRP_HIP(hipEventCreateWithFlags(&g->ev_done, hipEventDisableTiming));
		GRP_HIP(hipEventCreateWithFlags(&g->ev_keys, hipEventDisableTiming));
		GRP_HIP(hipEventCreateWithFlags(&g->ev_kdone, hipEventDisableTiming));
	}
	return MPM_OK;
}

}// namespace

extern "C" {

int mpm_group_unique_id(void* id128) {
	if(!id128) return MPM_ERR_INVALID;
	Rccl* r = rccl();
	if(!r) return MPM_ERR_DEVICE;
	static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
	return r->GetUniqueId(static_cast<ncclUniqueId*>(id128)) == ncclSuccess ? MPM_OK : MPM_ERR_DEVICE;
}

int mpm_group_create(mpm_ctx* ctx, int rank, int world, const void* id128, mpm_group** out) {
	if(!ctx || !out || world < 1 || world > 32 || rank < 0 || rank >= world || !id128) return MPM_ERR_INVALID;
	Rccl* r = rccl();
	if(!r) return fail(ctx, MPM_ERR_DEVICE, "librccl.so not found: multi-GPU groups need RCCL");
	mpm_group* g = new mpm_group();
	g->ctx = ctx, g->rank = rank, g->world = world;
	g->early_exchange = true;
	if(const char* e = getenv("MPM_GROUP_EARLY_EXCHANGE")) g->early_exchange = e[0] != '0';
	if(hipSetDevice(ctx->device) != hipSuccess) {
		delete g;
		return MPM_ERR_DEVICE;
	}
	ncclUniqueId id;
	memcpy(&id, id128, sizeof(id));
	const ncclResult_t nr = r->CommInitRank(&g->comm, world, id, rank);
	if(nr != ncclSuccess) {
		const std::string msg = std::string("ncclCommInitRank: ") + (r->GetErrorString ? r->GetErrorString(nr) : "error");
		delete g;
		return fail(ctx, MPM_ERR_DEVICE, msg);
	}
	if(r->CommCount) {// what RCCL itself says about the communicator: a caller (bench.py's log) can tell that it spans `world` ranks
		int n = 0;
		if(r->CommCount(g->comm, &n) == ncclSuccess && (n != world || getenv("MPM_GROUP_VERBOSE"))) fprintf(stderr, "claymore_hip: rank %d: ncclCommCount = %d (world %d)\n", rank, n, world);
		if(n && n != world) {
			if(r->CommAbort) r->CommAbort(g->comm);// (not a destroy: its peers may already be inside a collective of the communicator they think they have)
			else r->CommDestroy(g->comm);
			g->comm = nullptr;
			delete g;
			return fail(ctx, MPM_ERR_DEVICE, "ncclCommCount differs from the world size");
		}
	}
	const int rc = grp_common_init(g);
	if(rc) {
		mpm_group_destroy(g);
		return rc;
	}
	*out = g;
	return MPM_OK;
}

int mpm_group_create_local(mpm_ctx* const* ctxs, int world, mpm_group** out) {
	if(!ctxs || !out || world < 1 || world > 32) return MPM_ERR_INVALID;
	for(int p = 0; p < world; ++p)
		if(!ctxs[p]) return MPM_ERR_INVALID;
	LocalHub* hub = new LocalHub();
	hub->world	  = world;
	hub->refs	  = world;
	// Peer-direct transport (the reference's: one process, N devices, cudaMemcpyPeerAsync between them - mgsp_benchmark.cuh:309-356,
	// halo_buffer.cuh:54-59): when the contexts sit on different devices, peer access is enabled between every pair (Cuda.cu:120-127) and
	// the exchange runs in its asynchronous form - copies on the comm stream behind the peer's event, no host synchronisation, the same
	// ordering as the RCCL path.  MPM_GROUP_TRANSPORT=peer asks for that code path even on one device (how a one-GPU box tests it).
	bool multi = false;
	for(int p = 0; p < world; ++p) {
		hub->dev[p] = ctxs[p]->device;
		multi |= ctxs[p]->device != ctxs[0]->device;
	}
	const char* tr = getenv("MPM_GROUP_TRANSPORT");
	hub->peer_direct = multi || (tr && !strcmp(tr, "peer"));
	int caller_dev = 0;
	const bool have_dev = hipGetDevice(&caller_dev) == hipSuccess;
	if(multi) {
		for(int a = 0; a < world; ++a)
			for(int b = 0; b < world; ++b) {
				if(hub->dev[a] == hub->dev[b]) continue;
				int can = 0;
				if(hipSetDevice(hub->dev[a]) != hipSuccess || hipDeviceCanAccessPeer(&can, hub->dev[a], hub->dev[b]) != hipSuccess) can = 0;
				hipError_t e = can ? hipDeviceEnablePeerAccess(hub->dev[b], 0) : hipErrorPeerAccessUnsupported;
				if(e == hipErrorPeerAccessAlreadyEnabled) {
					(void) hipGetLastError();
					e = hipSuccess;
				}
				if(e != hipSuccess) {// no peer access between this pair: the runtime stages the copies (correct, slow) - said once
					if(hub->peer_direct) fprintf(stderr, "claymore_hip: no peer access from device %d to device %d (%s): copies between them are staged by the runtime\n", hub->dev[a], hub->dev[b], hipGetErrorString(e));
					hub->peer_direct = false;
				}
			}
	}
	if(multi && have_dev) (void) hipSetDevice(caller_dev);// (the pair loop walked over the devices: the caller's current device is its own business)
	if(getenv("MPM_GROUP_VERBOSE")) fprintf(stderr, "claymore_hip: in-process group of %d ranks on %s: %s transport\n", world, multi ? "several devices" : "one device", hub->peer_direct ? "peer-direct (hipMemcpyPeerAsync)" : "device-to-device copy");
	for(int p = 0; p < world; ++p) {
		mpm_group* g = new mpm_group();
		g->ctx = ctxs[p], g->rank = p, g->world = world, g->hub = hub;
		g->early_exchange = hub->peer_direct;// the asynchronous exchange is the peer-direct transport's form (no host waits for the GPU)
		if(const char* e = getenv("MPM_GROUP_EARLY_EXCHANGE")) g->early_exchange = e[0] != '0';// (tests: the RCCL ordering on the in-process transport)
		out[p] = g;
		const int rc = grp_common_init(g);
		if(rc) {
			for(int q = 0; q <= p; ++q) mpm_group_destroy(out[q]);
			return rc;
		}
	}
	return MPM_OK;
}

void mpm_group_destroy(mpm_group* g) {
	if(!g) return;
	if(g->ctx) hipSetDevice(g->ctx->device);
	if(g->ctx && g->ctx->group_refs > 0) g->ctx->group_refs--;
	hipDeviceSynchronize();
	if(getenv("MPM_GROUP_VERBOSE")) fprintf(stderr, "claymore_hip: rank %d of %d: %ld substeps in the group loop, %d key-list re-tags (a list outgrew its padding)\n", g->rank, g->world, (long) g->steps, g->retags);
	if(g->comm && rccl() && !g->aborted) rccl()->CommDestroy(g->comm);
	if(g->hub) {
		bool last;
		{
			std::lock_guard<std::mutex> lk(g->hub->m);
			last = --g->hub->refs == 0;
		}
		if(last) delete g->hub;
	}
	if(g->ev_sent) hipEventDestroy(g->ev_sent);
	if(g->ev_done) hipEventDestroy(g->ev_done);
	if(g->ev_keys) hipEventDestroy(g->ev_keys);
	if(g->ev_kdone) hipEventDestroy(g->ev_kdone);
	for(const SubstepEvents& ev: g->ev2)
		for(hipEvent_t e: {ev.start, ev.g2p2g_start, ev.g2p2g_end, ev.end})
			if(e) hipEventDestroy(e);
	delete g;
}

const char* mpm_group_transport(const mpm_group* g) {
	if(!g) return "";
	if(!g->hub) return "rccl";
	return g->hub->peer_direct ? "peer-direct" : "device-copy";
}
const char* mpm_group_last_error(const mpm_group* g) {
	return g ? g->err.c_str() : "null group";
}

// MgspBenchmark::initial_setup (mgsp_benchmark.cuh:561-659): per-rank setup, first tagging, initial rasterised grids summed once
int mpm_group_initial_setup(mpm_group* g) {
	if(!g || !g->ctx) return MPM_ERR_INVALID;
	g->ctx->group_summed = false;
	GRP_TRY(mpm_initial_setup(g->ctx));
	int rc = grp_tag(g);
	if(rc) return rc;
	rc = grp_exchange_halo(g, default_plan(g->ctx), 0, false);
	if(rc) return rc;
	GRP_TRY(mpm_sync(g->ctx));
	g->ctx->group_summed = true;
	return MPM_OK;
}

// Restart of a group (SURVEY 8f4: the checkpoint is what makes long multi-GPU runs possible): every rank has loaded ITS checkpoint into
// its context (mpm_checkpoint_load; taken at a substep boundary, i.e. after a call of this driver returned: the grid in it already holds
// the sum over the ranks).  What a checkpoint does not carry is rebuilt here, collectively: the padded key length, the overlap marks,
// the halo / interior lists and the per-peer send lists (grp_tag: all-gather of the block keys + tagging).
int mpm_group_resume(mpm_group* g) {
	if(!g || !g->ctx) return MPM_ERR_INVALID;
	g->ctx->group_summed = false;
	if(g->aborted) return gfail(g, MPM_ERR_DEVICE, "the RCCL communicator was aborted after an error");
	mpm_ctx* ctx = g->ctx;
	if(!ctx->ready) return gfail(g, MPM_ERR_NOT_READY, "mpm_group_resume: the context holds no state (initial set-up or mpm_checkpoint_load first)");
	ctx->group_summed = false;
	GRP_TRY(mpm_sync(ctx));
	ctx->halo_tagged = false;
	g->pad			 = 0;// (agreed on again from the ranks' block counts)
	int rc			 = grp_tag(g);
	if(rc) return rc;
	GRP_TRY(mpm_sync(ctx));
	ctx->group_summed = true;// (the checkpoint's grid is the sum: see above)
	return MPM_OK;
}

// One substep with ONE host synchronisation.  *max_vel_sqr = this rank's max |v|^2 after its grid update (not reduced).
// The enqueue half (everything up to the status read-back) and the wait half are separate: mpm_group_run_fixed puts the next
// substep's grid update and halo-first G2P2G between them.
namespace {
// plan.ev: the timing events this substep records (the windowed loop alternates two sets: a substep's events are read after the next
// substep's first half has been enqueued).  plan.counts_pending: the halo-first launch takes its block count from device memory.
int grp_substep_begin(mpm_group* g, const SubstepPlan& plan) {
	GRP_TRY(mgsp_begin(g->ctx, plan));
	return MPM_OK;
}
// everything of a substep behind the halo exchange: rebuild, key export, all-gather, tagging, the status read-back
int grp_substep_tail(mpm_group* g, const SubstepPlan& plan) {
	mpm_ctx* ctx  = g->ctx;
	const int pad = g->pad;
	int rc		  = grp_key_buffers(g);
	if(rc) return rc;
	if(g->overlap_tag) {
		// Round 5: the tagging chain - key all-gather, overlap marks / send lists, halo split - runs on the COMM stream beside the rebuild's last
		// kernel (prepare_blocks_kernel: list sort and look-up rows, 10-40 % of the rebuild; it shares nothing with the tagging but read-only
		// tables).  Everything the tagging and the status word read - both registrations, the carry-over's max |v|^2 slots, the rebuild's
		// counters - is complete when the keys are exported; the compute stream takes the tagging's results back before the status read-back.
		// OFF by default: with one rank alone on a GPU the two cross-stream events cost more than the overlap returns (1/8 slab of C3: 0.307-0.309 ms
		// per substep against 0.290-0.292 in line, 1/4: 0.443-0.445 against 0.425-0.427; profiles/r05_mgsp_rank_alone.txt) - the same finding as for
		// the grid carry-over on a second stream (DESIGN.md 5).  What it could hide on hardware is the key all-gather's latency across 8 GPUs, which
		// one GPU cannot show: MPM_GROUP_OVERLAP_TAG=1 keeps the path for that experiment (the MGSP suite passes with it on).
		for(hipEvent_t* e: {&ctx->ev_tag0, &ctx->ev_tag1})
			if(!*e) GRP_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
		StillLaunch rebuild_tail;
		GRP_TRY(mgsp_rebuild_export(ctx, plan, g->d_keys_mine, pad, &rebuild_tail));
		GRP_HIP(hipEventRecord(ctx->ev_tag0, ctx->s_compute));
		GRP_HIP(hipStreamWaitEvent(ctx->s_comm, ctx->ev_tag0, 0));
		GRP_TRY(launch_rebuild_prepare(ctx, rebuild_tail));
		rc = grp_all_gather(g, g->d_keys_mine, g->d_keys_all, 3 * (size_t) pad, ctx->s_comm);
		if(rc) return rc;
		GRP_TRY(mgsp_tag(ctx, plan, g->d_keys_all, pad, g->world, g->rank, ctx->s_comm));
		GRP_HIP(hipEventRecord(ctx->ev_tag1, ctx->s_comm));
		GRP_HIP(hipStreamWaitEvent(ctx->s_compute, ctx->ev_tag1, 0));
		GRP_HIP(hipEventRecord(plan.ev.end, ctx->s_compute));
	} else {
		GRP_TRY(mgsp_rebuild_export(ctx, plan, g->d_keys_mine, pad, nullptr));
		rc = grp_all_gather(g, g->d_keys_mine, g->d_keys_all, 3 * (size_t) pad, ctx->s_compute);
		if(rc) return rc;
		GRP_TRY(mgsp_tag(ctx, plan, g->d_keys_all, pad, g->world, g->rank));
	}
	GRP_TRY(mgsp_end_enqueue(ctx, plan));
	g->pad_enqueued = pad;
	return MPM_OK;
}
int grp_substep_enqueue(mpm_group* g, const SubstepPlan& plan) {
	int rc = grp_exchange_halo(g, plan, 1, true);
	return rc ? rc : grp_substep_tail(g, plan);
}
// takes over the counts of the substep whose read-back is outstanding (timed from ev.start); truncated: a key list outgrew the padding it
// was exported with
int grp_substep_wait(mpm_group* g, const SubstepEvents& ev, float* max_vel_sqr, bool* truncated) {
	mpm_ctx* ctx = g->ctx;
	int mx		 = 0;
	float mv	 = 0.f;
	GRP_TRY(mgsp_end_wait(ctx, g->rank, g->send_counts, &g->n_halo_blocks, &mx, &mv, ev));
	g->send_counts[g->rank] = 0;
	if(max_vel_sqr) *max_vel_sqr = mv;
	g->g2p2g_ms_sum += ctx->last_g2p2g_ms;
	g->steps++;
	const int pad = g->pad_enqueued;
	*truncated	  = mx > pad;
	if(*truncated || grp_pad_close(g, mx, pad)) g->pad = std::max(g->pad, grp_pad_for(g, mx));// truncated, or close: the same new length on every rank (they all see the same row 0s); takes effect at the next export
	return MPM_OK;
}
}// namespace

int mpm_group_substep(mpm_group* g, float dt, float next_dt, float* max_vel_sqr) {
	if(!g || !g->ctx) return MPM_ERR_INVALID;
	g->ctx->group_summed = false;
	const SubstepPlan plan = mgsp_plan(g->ctx, dt, next_dt);
	int rc				   = grp_substep_begin(g, plan);
	if(rc) return rc;
	rc = grp_substep_enqueue(g, plan);
	if(rc) return rc;
	bool truncated = false;
	rc			   = grp_substep_wait(g, plan.ev, max_vel_sqr, &truncated);
	if(rc) return rc;
	if(truncated) {// a key list was truncated (same verdict on every rank): tag again with the larger padding
		g->retags++;
		if((rc = grp_tag(g))) return rc;
	}
	g->ctx->group_summed = true;
	return MPM_OK;
}

// nsteps substeps with a fixed dt.  The host does not wait at the end of a substep: the status read-back of substep t (the counts of its
// tagging - the sizes of the next ncclSend / ncclRecv -, every rank's status word) is waited for AFTER the grid update and the
// halo-first G2P2G of substep t + 1 have been enqueued (they take their counts from device memory), so the GPU works on those while the
// host wakes up, looks at the counts and enqueues the exchange.  A rank that fails is seen by every rank at the same read-back (row 0 of
// the key all-gather carries its status word): all return the error, nobody is left waiting in a collective.
int mpm_group_run_fixed(mpm_group* g, int nsteps, float dt) {
	if(!g || !g->ctx) return MPM_ERR_INVALID;
	mpm_ctx* ctx	  = g->ctx;
	ctx->group_summed = false;
	bool pending = false;// the read-back of the previous substep is outstanding
	bool retagged = false;// the wait half had to repeat the last tagging (a key list outgrew its padding)
	bool lean_prev_end = false;// (lean events) the previous substep of this run recorded its end event: the next one is timed from it
	// The deferred order needs the exchange in its RCCL ordering (collect on the compute stream in front of the interior launch); the
	// in-process transport's default (interior first, host synchronisations inside the exchange) keeps one wait per substep.
	const bool defer = !g->no_defer && g->early_exchange;
	const bool lean	 = defer && !g->overlap_tag;// (the deferred order records the halo event itself; the overlapped tagging keeps its own end event)
	auto bail = [&](int rc) {// an interrupted run leaves no promise about the grid behind (FlagGuard), and no read-back in flight
		FlagGuard guard {ctx};
		if(pending) hipEventSynchronize(ctx->ev_pending ? ctx->ev_pending : ctx->ev_status);
		return rc;
	};
	auto finish = [&](int par, bool may_retag) {// the wait half of a substep
		// (lean events: no start event - a substep is timed from the end of the one before it, the first of a run from its G2P2G start)
		SubstepEvents ev = g->ev2[par];
		if(lean) ev.start = lean_prev_end ? g->ev2[par ^ 1].end : ev.g2p2g_start;
		lean_prev_end  = lean;
		float mv	   = 0.f;
		bool truncated = false;
		int rc		   = grp_substep_wait(g, ev, &mv, &truncated);
		pending		   = false;
		if(rc == MPM_OK && (std::isinf(mv) || std::isnan(mv))) rc = gfail(g, MPM_ERR_NONFINITE, "Maximum velocity is infinity");
		if(rc == MPM_OK && truncated) {
			// A key list outgrew its padding (rare: the padding grows at 3/4 fill): the tagging of that substep missed blocks - the same verdict on
			// every rank.  Where the host waits at the end of the substep nothing has run on it yet: tag again.  In the deferred order the next
			// substep's two G2P2G passes are already enqueued on it; they are still RIGHT - a particle block is done by exactly one of them
			// whatever the overlap marks say, and they add into this rank's own grid - what is incomplete is the send lists the collect ran
			// with.  So: wait for both passes (the interior launch reads the flags the new tagging rewrites), tag again, and let the comm half
			// collect once more with the complete lists.  (Round 4 gave up here with MPM_ERR_CAPACITY.)
			if(!may_retag) GRP_HIP(hipStreamSynchronize(ctx->s_compute));
			rc = grp_tag(g);
			g->retags++;
			retagged = true;
		}
		return rc;
	};
	for(int i = 0; i < nsteps; ++i) {
		const int par = i & 1;
		SubstepPlan plan {dt, dt, g->ev2[par]};
		// the next substep's dt is known: its grid update rides on this substep's carry-over (carry_grid_kernel<true>, which writes the
		// max |v|^2 slots: this substep's clear resets them); the last substep of the call leaves the canonical state behind
		if(i + 1 < nsteps) plan.fuse_dt = dt;
		plan.rebuild_clear = true, plan.counts_pending = pending, plan.lean_events = lean;
		int rc = grp_substep_begin(g, plan);// (its own grid update rode on the previous substep's carry-over)
		if(rc) return bail(rc);
		if(defer) {
			if((rc = grp_halo_compute_half(g, plan, 1))) return bail(rc);
			retagged = false;
			if(pending && (rc = finish(par ^ 1, false))) return bail(rc);// the GPU is busy with the interior launch while the host looks at the counts
			if((rc = grp_halo_comm_half(g, 1, retagged)) || (rc = grp_substep_tail(g, plan))) return bail(rc);
		} else {
			if((rc = grp_substep_enqueue(g, plan))) return bail(rc);
		}
		pending = true;
		if((!defer || i + 1 == nsteps) && (rc = finish(par, true))) return bail(rc);
	}
	ctx->group_summed = true;// (the last carry-over is not fused: grid[0] holds the summed momentum)
	return MPM_OK;
}

// compute_dt of the MGSP project (Projects/MGSP/utility_funcs.hpp:32-55): CFL 0.3 and the 0.51 frame-remainder rule
float mpm_group_compute_dt(const mpm_group* g, float max_vel, float cur, float next, float dt_default) {
	if(!g || !g->ctx) return 0.f;
	if(next < cur) return 0.f;
	float dt = dt_default;
	if(max_vel > 0.f) {
		max_vel = g->ctx->g.dx * 0.3f / max_vel;
		if(max_vel < dt_default) dt = max_vel;
	}
	if(cur + dt >= next) {
		dt = next - cur;
	} else {
		max_vel = (next - cur) * 0.51f;
		if(max_vel < dt) dt = max_vel;
	}
	return dt;
}

// MgspBenchmark::main_loop (mgsp_benchmark.cuh:361-559) for `frames` frames of 1 / fps seconds: adaptive dt from the maximum
// grid velocity over ALL ranks (:410-418).  on_frame (may be null) is called after every frame (the reference writes its
// particle files there).  *steps_out receives the number of substeps taken.
int mpm_group_main_loop(mpm_group* g, int frames, int fps, float dt_default, void (*on_frame)(int frame, void* user), void* user, int* steps_out) {
	if(!g || !g->ctx || frames < 0 || fps < 1) return MPM_ERR_INVALID;
	mpm_ctx* ctx			= g->ctx;
	ctx->group_summed		= false;
	const float seconds_pf	= 1.f / (float) fps;
	float next_dt			= mpm_group_compute_dt(g, 0.f, 0.f, seconds_pf, dt_default);
	int steps				= 0;
	for(int frame = 1; frame <= frames; ++frame) {
		const float next_time = seconds_pf;// per-frame clock, as in the reference (:375-380)
		float cur_time		  = 0.f;
		while(cur_time < next_time) {
			const float dt = next_dt;
			if(!(dt > 0.f)) return gfail(g, MPM_ERR_INVALID, "time step is not positive");
			// grid update first: the next dt needs the maximum velocity of all ranks (:388-418)
			float mv2 = 0.f;
			GRP_TRY(mpm_grid_update(ctx, dt, &mv2));
			int rc = grp_all_reduce_max(g, &mv2);
			if(rc) return rc;
			if(std::isinf(mv2) || std::isnan(mv2)) return gfail(g, MPM_ERR_NONFINITE, "Maximum velocity is infinity");
			next_dt = mpm_group_compute_dt(g, std::sqrt(mv2), cur_time + dt, next_time, dt_default);
			if(!(next_dt > 0.f)) next_dt = mpm_group_compute_dt(g, std::sqrt(mv2), 0.f, seconds_pf, dt_default);// first dt of the next frame
			GRP_TRY(mpm_g2p2g_halo(ctx, dt, next_dt));
			rc = grp_exchange_halo(g, default_plan(ctx, dt, next_dt), 1, true);
			if(rc) return rc;
			GRP_TRY(mpm_rebuild_partition(ctx, nullptr));
			rc = grp_tag(g);
			if(rc) return rc;
			g->g2p2g_ms_sum += ctx->last_g2p2g_ms;
			g->steps++;
			steps++;
			cur_time += dt;
		}
		ctx->group_summed = true;// (an unfused rebuild behind the summing exchange: the group readout may run inside on_frame)
		if(on_frame) on_frame(frame, user);
	}
	if(steps_out) *steps_out = steps;
	return MPM_OK;
}

// ---- readout of a group (an extension: mpm_readout.hpp) ----------------------------------------------------------------
// At the return of a group call that completed, and inside mpm_group_main_loop's on_frame, every rank's grid[0] holds the mass and
// momentum summed over the ranks on every node its own particles reach: the halo exchange reduces the peers' shares of each shared block
// into grid[1] before the rebuild's carry-over copies it into grid[0] (and the set-up exchange sums the rasterised grids in grid[0]).
// So the single-context readout, run on each rank's own grid, reads the group's velocity field; tests/test_group_velocity_gpu.py
// checks the premise node by node against a single context.
// A readout error leaves the group as it is (gfail would break an in-process group's rendez-vous for good): it is only reported.
static int grp_readout_fail(mpm_group* g, int code, const std::string& msg) {
	g->err = g->ctx->err = msg;
	return code;
}
static int grp_readout_state(mpm_group* g, const char* who) {
	mpm_ctx* ctx = g->ctx;
	if(!ctx->ready) return grp_readout_fail(g, MPM_ERR_NOT_READY, std::string(who) + ": the context holds no state (mpm_group_initial_setup first)");
	if(!ctx->group_summed)
		return grp_readout_fail(g, MPM_ERR_INVALID, std::string(who) + ": the grid does not hold the group's summed momentum - a group call failed, or a phase-level call ran on the context since the last group call completed");
	if(!ctx->grid_momentum) return grp_readout_fail(g, MPM_ERR_INVALID, std::string(who) + ": the grid holds velocities");
	return MPM_OK;
}

int mpm_group_retrieve_velocity(mpm_group* g, int model, float* xyz, float* vel, float* affine9, size_t* n) {
	if(!g || !g->ctx) return MPM_ERR_INVALID;
	mpm_ctx* ctx = g->ctx;
	if(int rc = grp_readout_state(g, "mpm_group_retrieve_velocity")) return rc;
	if(model < 0 || model >= (int) ctx->models.size() || !n || !xyz || !vel) return grp_readout_fail(g, MPM_ERR_INVALID, "mpm_group_retrieve_velocity: bad model or NULL output array");
	if(int rc = readout_velocity(ctx, model, xyz, vel, affine9, n)) return grp_readout_fail(g, rc, ctx->err);
	return MPM_OK;
}

// Collective: every rank contributes its status and its five float64 sums to one all-gather (12 ints per rank: status, 0, the sums as
// 10 ints) - grp_all_gather, the one collective every transport has - and each rank adds the sums on the host in rank order, so all
// ranks return the same bits.  A rank that cannot read out still takes part: its status fails the call on every rank.
int mpm_group_particle_momentum(mpm_group* g, int model, double out[5]) {
	if(!g || !g->ctx) return MPM_ERR_INVALID;
	mpm_ctx* ctx = g->ctx;
	constexpr int kRow = 2 + 2 * kMomentumSums;
	int row[kRow] = {};
	double mine[kMomentumSums] = {};
	int rc = grp_readout_state(g, "mpm_group_particle_momentum");
	if(!rc && (model < -1 || model >= (int) ctx->models.size() || !out)) rc = grp_readout_fail(g, MPM_ERR_INVALID, "mpm_group_particle_momentum: bad model or NULL output array");
	if(!rc && (rc = readout_momentum(ctx, model, mine))) grp_readout_fail(g, rc, ctx->err);
	const std::string mine_err = g->err;
	row[0] = rc;
	memcpy(row + 2, mine, sizeof(mine));
	GRP_HIP(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	DevBuf<int> d_row, d_all;
	GRP_HIP(d_row.alloc(kRow, s));
	GRP_HIP(d_all.alloc((size_t) kRow * g->world, s));
	GRP_HIP(hipMemcpyAsync(d_row.p, row, sizeof(row), hipMemcpyHostToDevice, s));
	const int grc = grp_all_gather(g, d_row.p, d_all.p, kRow, s);
	if(grc) return rc ? grp_readout_fail(g, rc, mine_err) : grc;// (a group that a failed call left broken: this rank's own reason first)
	std::vector<int> all((size_t) kRow * g->world);
	GRP_HIP(hipMemcpyAsync(all.data(), d_all.p, sizeof(int) * all.size(), hipMemcpyDeviceToHost, s));
	GRP_HIP(hipStreamSynchronize(s));
	if(g->hub && g->hub->have_kdone)// (asynchronous in-process gather: a peer may still be copying d_row, which goes out of scope here)
		for(int p = 0; p < g->world; ++p)
			if(p != g->rank && g->hub->ev_kdone[p]) GRP_HIP(hipEventSynchronize(g->hub->ev_kdone[p]));
	if(rc) return grp_readout_fail(g, rc, mine_err);
	double sum[kMomentumSums] = {};
	for(int p = 0; p < g->world; ++p) {
		const int* r = all.data() + (size_t) kRow * p;
		if(r[0]) return grp_readout_fail(g, r[0], "mpm_group_particle_momentum: rank " + std::to_string(p) + " could not read out its particles");
		double d[kMomentumSums];
		memcpy(d, r + 2, sizeof(d));
		for(int k = 0; k < kMomentumSums; ++k) sum[k] += d[k];
	}
	for(int k = 0; k < kMomentumSums; ++k) out[k] = sum[k];
	return MPM_OK;
}

int mpm_group_stats(const mpm_group* g, int* send_counts32, int* halo_particle_blocks, float* g2p2g_ms_avg) {
	if(!g) return MPM_ERR_INVALID;
	if(send_counts32)
		for(int p = 0; p < 32; ++p) send_counts32[p] = p < g->world && p != g->rank ? g->send_counts[p] : 0;
	if(halo_particle_blocks) *halo_particle_blocks = g->n_halo_blocks;
	if(g2p2g_ms_avg) *g2p2g_ms_avg = g->steps ? (float) (g->g2p2g_ms_sum / (double) g->steps) : 0.f;
	return MPM_OK;
}

}// extern "C"
