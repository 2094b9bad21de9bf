// mpm_halo.inc — MGSP static-particle-partition halo path (Projects/MGSP/halo_kernels.cuh, mgsp_benchmark.cuh:661-776).
// Included at the end of claymore_hip.hip.  Transport (all-gather of keys, all-to-all of halo blocks) is done by the
// caller over RCCL on the buffers it hands in; this file holds the kernels on either side of it.
//
// A neighbor block is "overlapping" with peer p iff it is a NEIGHBOR block (index < nbc) on both ranks, which makes the
// relation symmetric: what I send to p is exactly what p sends to me, so receive counts equal send counts and no count
// exchange is needed.  (The reference also tags blocks that are only exterior on one side, halo_kernels.cuh:28-33, and
// then ships their stale contents; an exterior-only block holds no contribution, so leaving it out changes nothing.)
namespace mpm {

// The tagging kernels run on device-sized counts: every count is read from device memory, launches are sized by host-known upper bounds,
// so nothing has to be read back between the rebuild and the tagging of a fused substep.
// Row 0 of the exported list = {true key count, this rank's STATUS WORD, 0}: every rank sees every rank's status in the same substep
// (halo_mark_kernel records it), so a rank that failed - block / list / bin capacity exceeded, non-finite velocity - does not leave
// its peers waiting in the next collective: all ranks return the error at the same synchronisation.  Bits: kPeerErr*.
// The kernel also clears what the tagging that follows accumulates into - the overlap marks and the halo counters (they must outlive
// the substep's halo-first G2P2G and its collect / reduce kernels, which read them: they used to be cleared before G2P2G, when the
// host held a copy of every count).
enum { kPeerErrBlocks = 1, kPeerErrList = 2, kPeerErrBins = 4, kPeerErrNonfinite = 8, kPeerErrBooks = 16 /* bucketed + lost + dropped != added (check_books) */ };
__global__ void halo_export_kernel(int cap, const int* __restrict__ status, const unsigned* __restrict__ max_vel_bits, int drop_overflow, long long books_expected, const int* __restrict__ keys, int* out, int pad_rows, int* overlap, int overlap_n, int* halo_counts, int halo_counts_n) {
	__shared__ int s_bad;
	if(blockIdx.x == 0) {// (workgroup 0 forms the status word; the branch is uniform per workgroup)
		if(threadIdx.x == 0) s_bad = 0;
		__syncthreads();
		if(threadIdx.x < kMaxVelSlots && max_vel_bits[threadIdx.x * kMaxVelStride] >= 0x7f800000u) atomicOr(&s_bad, 1);// inf marks a NaN velocity (grid update)
		__syncthreads();
	}
	const int nbc = status[ST_NBC];// (the true count is exported even when it exceeds the capacity: the host reports that)
	const int n	  = min(min(nbc, cap), pad_rows - 1);
	for(int i = blockIdx.x * blockDim.x + threadIdx.x; i < 3 * pad_rows; i += gridDim.x * blockDim.x) {
		const int row = i / 3, c = i - 3 * row;
		int v		  = row <= n ? keys[3 * (row - 1 < 0 ? 0 : row - 1) + c] : 0;
		if(row == 0) {
			v = 0;
			if(c == 0) v = nbc;
			if(c == 1) {// (blockIdx.x == 0 here: i == 1)
				const int ov = status[ST_OVERFLOW];
				v = (ov & 1 ? kPeerErrBlocks : 0) | ((ov & 2) && !drop_overflow ? kPeerErrList : 0) | (ov & 4 ? kPeerErrBins : 0) | ((status[ST_NONFINITE] || s_bad) ? kPeerErrNonfinite : 0)
					| (nbc > cap ? kPeerErrBlocks : 0);
				// the rank's particle books (check_books on the host): the rebuild's totals are complete by now
				long long held = (long long) status[ST_LOST] + (long long) status[ST_DROPPED];
				for(int m = 0; m < kMaxModels; ++m) held += (long long) status[ST_PART0 + m];
				if(v == 0 && held != books_expected) v |= kPeerErrBooks;
			}
		}
		out[i] = v;
	}
	for(int i = blockIdx.x * blockDim.x + threadIdx.x; i < overlap_n; i += gridDim.x * blockDim.x) overlap[i] = 0;
	for(int i = blockIdx.x * blockDim.x + threadIdx.x; i < halo_counts_n; i += gridDim.x * blockDim.x) halo_counts[i] = 0;
}

// mark_overlapping_blocks, halo_kernels.cuh:21-35.  All peers in ONE launch (blockIdx.y = peer - peer0): at 8 ranks one launch per peer
// was 7 kernels + 8 four-byte copies, ~75 us of launch latency at the end of every substep, where nothing overlaps it.
//   n_in < 0: the all-gathered lists, pad_rows rows per peer behind a row 0 of halo_export_kernel's; records every rank's key-list
//             length and status word in peer_len.
//   n_in >= 0: the n_in keys of peer peer0 at rows, without a header (mpm_halo_tag_peer: one peer, the count from the host).
// table: the partition whose neighbor blocks are marked (status[ST_NBC] holds its count).
struct PeerSendLists {
	int* ids[32];
};
__global__ void halo_mark_kernel(GridCfg cfg, const int* __restrict__ rows, int pad_rows, int n_in, int peer0, int rank, const int* __restrict__ table, const int* __restrict__ status, int* overlap, PeerSendLists send, int* send_counts /* [32] */, int* peer_len /* [world], [32 + world] */) {
	const int peer	= peer0 + blockIdx.y;
	const int* keys = rows;
	if(n_in < 0) {
		const int* peer_rows = rows + (size_t) 3 * pad_rows * peer;
		if(blockIdx.x == 0 && threadIdx.x == 0) {
			peer_len[peer]		= peer_rows[0];
			peer_len[32 + peer] = peer_rows[1];// the peer's status word (halo_export_kernel)
		}
		if(peer == rank) return;
		n_in = min(peer_rows[0], pad_rows - 1);
		keys = peer_rows + 3;
	}
	const int nbc = min(status[ST_NBC], cfg.cap);
	const int i	  = blockIdx.x * blockDim.x + threadIdx.x;
	int b		  = -1;
	if(i < n_in) b = table_query(cfg, table, keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]);
	const bool hit = b >= 0 && b < nbc;
	const int slot = wave_append(&send_counts[peer], hit);
	if(hit) {
		atomicOr(&overlap[b], 1 << peer);
		send.ids[peer][slot] = b;
	}
}

// collect_blockids_for_halo_reduction, halo_kernels.cuh:37-62: a particle block is "halo" if any of its 2^3 grid blocks
// is shared with a peer; the halo blocks are listed (halo-first launch), the others flagged (interior launch over all blocks).
// keys / table: the partition whose particle blocks are split (status[ST_PBC] holds its count).
__global__ void halo_split_kernel(GridCfg cfg, const int* __restrict__ status, const int* __restrict__ keys, const int* __restrict__ table, const int* __restrict__ overlap, int* halo_list, int* inner_list, int* counts) {
	const int pbc = min(status[ST_PBC], cfg.cap);
	for(int b0 = blockIdx.x * blockDim.x; b0 < pbc; b0 += gridDim.x * blockDim.x) {// uniform trip count per workgroup (block_append has barriers)
		const int b		 = b0 + threadIdx.x;
		const bool valid = b < pbc;
		bool halo		 = false;
		if(valid) {
			const int kx = keys[3 * b], ky = keys[3 * b + 1], kz = keys[3 * b + 2];
			for(int i = 0; i < 2; ++i)
				for(int j = 0; j < 2; ++j)
					for(int k = 0; k < 2; ++k) {
						const int nb = table_query(cfg, table, kx + i, ky + j, kz + k);
						if(nb >= 0 && overlap[nb]) halo = true;
					}
		}
		// (the two counters share a cache line: one atomic each per workgroup, not per wave - same-line atomics serialise in L2)
		const int sh = block_append(&counts[0], valid && halo ? 1 : 0);
		block_append(&counts[1], valid && !halo ? 1 : 0);
		if(valid && halo) halo_list[sh] = b;
		if(valid) inner_list[b] = halo ? 0 : 1;// a flag per block: the interior pass runs over all blocks in their own order and skips the halo ones
	}
}

// collect_grid_blocks, halo_kernels.cuh:64-80: one wave per block, lane = cell.  All peers in one launch (blockIdx.y = peer - peer0),
// every size read from device memory - the send counts of the last tagging and, from them, each peer's segment of the send buffer
// (segments in peer order, kHaloRow floats per block: the layout the host derives from the same counts for ncclSend / ncclRecv) -, so
// that the collect can be enqueued before the host has read those counts back.  A segment that does not fit into the buffer is left
// out (the host sees the same counts, grows the buffer and collects again).
// one_keys != null: one peer (peer0) into the caller's separate key and block arrays (mpm_halo_collect; out_cap_floats bounds the two).
constexpr size_t kHaloRow = 3 + 256;// one halo record: key (3 x int32) + grid block (4 x 64 x f32)
__global__ __launch_bounds__(256) void halo_collect_kernel(const int* __restrict__ send_counts /* [32] */, int peer0, int rank, PeerSendLists ids, const int* __restrict__ keys, const float* __restrict__ grid, float* out, size_t out_cap_floats, int* one_keys, float* one_blocks) {
	const int peer = peer0 + blockIdx.y;
	if(peer == rank) return;
	const int n = send_counts[peer];
	if(n <= 0) return;
	size_t off = 0;
	if(!one_keys)
		for(int q = 0; q < peer; ++q)
			if(q != rank) off += kHaloRow * (size_t) send_counts[q];
	if(off + kHaloRow * (size_t) n > out_cap_floats) return;
	int* out_keys	  = one_keys ? one_keys : reinterpret_cast<int*>(out + off);
	float* out_blocks = one_keys ? one_blocks : out + off + 3 * (size_t) n;
	const int lane	  = threadIdx.x & 63;
	for(int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
		const int b	   = ids.ids[peer][i];
		const float* s = grid + (size_t) b * 256;
		float* d	   = out_blocks + (size_t) i * 256;
		d[lane]		   = s[lane];
		d[64 + lane]   = s[64 + lane];
		d[128 + lane]  = s[128 + lane];
		d[192 + lane]  = s[192 + lane];
		if(lane < 3) out_keys[3 * i + lane] = keys[3 * b + lane];
	}
}

// reduce_grid_blocks, halo_kernels.cuh:82-97.  A zero addend (+0 or -0) is skipped, which saves the atomics of the empty half of a shared block.
// That is the float32 sum bit for bit except for one combination: +0 added to a node that holds -0 leaves -0 where the IEEE sum is +0.  No entry
// point puts a -0 into a grid (it is cleared to +0, and a sum of +0 and normal values in round-to-nearest is never -0; a -0 addend is skipped
// here), and the two zeros compare equal everywhere the grid is read.
__global__ __launch_bounds__(256) void halo_reduce_kernel(GridCfg cfg, int n, const int* __restrict__ in_keys, const float* __restrict__ in_blocks, const int* __restrict__ table, int nbc, float* grid) {
	const int i	   = blockIdx.x * 4 + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if(i >= n) return;
	const int b = table_query(cfg, table, in_keys[3 * i], in_keys[3 * i + 1], in_keys[3 * i + 2]);
	if(b < 0 || b >= nbc) return;
	const float* s = in_blocks + (size_t) i * 256;
	float* d	   = grid + (size_t) b * 256;
#pragma unroll
	for(int ch = 0; ch < 4; ++ch) {
		const float v = s[ch * 64 + lane];
		if(v != 0.f) unsafeAtomicAdd(d + ch * 64 + lane, v);
	}
}

}// namespace mpm

static int halo_alloc(mpm_ctx* ctx) {
	if(ctx->d_overlap) return MPM_OK;
	HIP_TRY(alloc_block_array(ctx, ctx->d_halo_list));
	HIP_TRY(alloc_block_array(ctx, ctx->d_inner_list));
	HIP_TRY(alloc_block_array(ctx, ctx->d_overlap));// (last: the three exist together)
	// (the halo counters and the peers' key-list lengths live in the status block: they come back with the one read-back of a synchronisation)
	for(int p = 0; p < 32; ++p) ctx->h_peer_rows[p] = 0;
	return MPM_OK;
}

// The launches of the tagging.  part: the partition they read - the current one (set-up, resume, a re-tag, the phase calls) or the one
// just rebuilt (mgsp_rebuild_export / mgsp_tag, in the substep that rebuilds it); status[ST_PBC] / [ST_NBC] hold its counts either way.
// halo_export: this rank's key list into dev_keys (pad_rows rows, row 0 = {count, status word, 0}); clears the overlap marks and counters.
static int halo_export(mpm_ctx* ctx, int part, int* dev_keys, int pad_rows) {
	long long books_expected = -ctx->books_bias;
	for(auto& m: ctx->models) books_expected += (long long) m.n;
	halo_export_kernel<<<std::min(1024u, cdiv((size_t) 3 * pad_rows, 256)), 256, 0, ctx->s_compute>>>(ctx->g.cap, ctx->d_status, ctx->d_maxvel, ctx->cfg.drop_overflow, books_expected, ctx->part[part].keys, dev_keys, pad_rows, ctx->d_overlap,
																										 ctx->g.cap + 1, ctx->d_halo_counts, 2 + 32);
	HIP_TRY(hipGetLastError());
	return MPM_OK;
}
static int halo_send_lists(mpm_ctx* ctx, PeerSendLists* send, int peer0, int npeers, int rank) {
	*send = PeerSendLists {};
	for(int p = peer0; p < peer0 + npeers; ++p) {
		if(p == rank) continue;
		if(!ctx->d_send_ids[p]) HIP_TRY(alloc_block_array(ctx, ctx->d_send_ids[p]));
		send->ids[p] = ctx->d_send_ids[p];
	}
	return MPM_OK;
}
static void launch_halo_split(mpm_ctx* ctx, int part, hipStream_t s) {
	halo_split_kernel<<<std::max(1u, std::min(2048u, cdiv(ctx->ebc, 256))), 256, 0, s>>>(ctx->g, ctx->d_status, ctx->part[part].keys, ctx->part[part].table, ctx->d_overlap, ctx->d_halo_list, ctx->d_inner_list, ctx->d_halo_counts);
}
// overlap marks / send lists / halo split from the all-gathered key lists (world * pad_rows rows), on stream s
static int halo_tag(mpm_ctx* ctx, int part, const int* dev_all_keys, int pad_rows, int world, int rank, hipStream_t s) {
	PeerSendLists send;
	int rc = halo_send_lists(ctx, &send, 0, world, rank);
	if(rc) return rc;
	halo_mark_kernel<<<dim3(cdiv(pad_rows, 256), world), 256, 0, s>>>(ctx->g, dev_all_keys, pad_rows, -1, 0, rank, ctx->part[part].table, ctx->d_status, ctx->d_overlap, send, &ctx->d_halo_counts[2], ctx->d_peer_rows);
	launch_halo_split(ctx, part, s);
	HIP_TRY(hipGetLastError());
	return MPM_OK;
}
// the counts of the last tagging, read back (h_halo_counts) and taken over
static void halo_take_counts(mpm_ctx* ctx) {
	ctx->n_halo	 = ctx->h_halo_counts[0];
	ctx->n_inner = ctx->h_halo_counts[1];
	for(int p = 0; p < 32; ++p) ctx->send_count[p] = ctx->h_halo_counts[2 + p];
	ctx->halo_tagged = true;
}
// one read-back of the halo counters (and of the first `world` key-list lengths behind them) on the compute stream
static int halo_read_counts(mpm_ctx* ctx, int world) {
	hipStream_t s = ctx->s_compute;
	HIP_TRY(hipMemcpyAsync(ctx->h_halo_counts, ctx->d_halo_counts, sizeof(int) * (2 + 32 + world), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	halo_take_counts(ctx);
	return MPM_OK;
}

extern "C" {

int mpm_halo_keys(mpm_ctx* ctx, int* dev_keys, int capacity_blocks, int* count) {
	phase_call(ctx);
	if(!ctx || !ctx->ready || !dev_keys) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	const int ncopy = std::min(ctx->nbc, capacity_blocks);// *count reports the true number; the caller retries if truncated
	if(ncopy > 0) HIP_TRY(hipMemcpyAsync(dev_keys, ctx->part[ctx->rollid].keys, sizeof(int) * 3 * (size_t) ncopy, hipMemcpyDeviceToDevice, ctx->s_compute));
	if(count) *count = ctx->nbc;
	return MPM_OK;
}

int mpm_halo_tag_begin(mpm_ctx* ctx) {
	phase_call(ctx);
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(ctx->body_mask) return fail(ctx, MPM_ERR_INVALID, "mpm_halo_tag_begin: the context has a rigid body (mpm_set_collider_body); bodies in multi-GPU groups are not computed");
	if(ctx->force.count) return fail(ctx, MPM_ERR_INVALID, "mpm_halo_tag_begin: the context has a force field (mpm_set_force_field); force fields in multi-GPU groups are not computed");
	HIP_TRY(hipSetDevice(ctx->device));
	int rc = halo_alloc(ctx);
	if(rc) return rc;
	HIP_TRY(hipMemsetAsync(ctx->d_overlap, 0, sizeof(int) * ((size_t) ctx->nbc + 1), ctx->s_compute));
	HIP_TRY(hipMemsetAsync(ctx->d_halo_counts, 0, sizeof(int) * (2 + 32), ctx->s_compute));
	ctx->halo_tagged = false;
	return MPM_OK;
}

int mpm_halo_tag_peer(mpm_ctx* ctx, int peer, const int* dev_peer_keys, int npeer_keys) {
	phase_call(ctx);
	if(!ctx || !ctx->ready || !ctx->d_overlap || peer < 0 || peer >= 32) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	PeerSendLists send;
	int rc = halo_send_lists(ctx, &send, peer, 1, -1);
	if(rc) return rc;
	if(npeer_keys > 0)
		halo_mark_kernel<<<cdiv(npeer_keys, 256), 256, 0, ctx->s_compute>>>(ctx->g, dev_peer_keys, 0, npeer_keys, peer, -1, ctx->part[ctx->rollid].table, ctx->d_status, ctx->d_overlap, send, &ctx->d_halo_counts[2], nullptr);
	return MPM_OK;
}

int mpm_halo_tag_end(mpm_ctx* ctx, int* halo_particle_blocks, int* send_counts) {
	phase_call(ctx);
	if(!ctx || !ctx->ready || !ctx->d_overlap) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	launch_halo_split(ctx, ctx->rollid, ctx->s_compute);
	int rc = halo_read_counts(ctx, 0);
	if(rc) return rc;
	if(halo_particle_blocks) *halo_particle_blocks = ctx->n_halo;
	if(send_counts)
		for(int p = 0; p < 32; ++p) send_counts[p] = ctx->send_count[p];
	return MPM_OK;
}

// plan.rebuild_clear: mpm_mgsp_begin ... mpm_mgsp_rebuild_export.  plan.counts_pending: the number of halo blocks is read from device memory,
// ctx->n_halo is then an estimate that sizes the launch.  plan.ev.g2p2g_start marks the start.
static int g2p2g_halo(mpm_ctx* ctx, const SubstepPlan& plan) {
	if(!ctx || !ctx->ready || !ctx->halo_tagged) return MPM_ERR_NOT_READY;
	FlagGuard guard {ctx};
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	int rc		  = launch_g2p2g_prologue(ctx, plan);
	if(rc) return rc;
	HIP_TRY(hipEventRecord(plan.ev.g2p2g_start, s));
	if(plan.counts_pending || ctx->n_halo)
		for(auto& m: ctx->models) launch_g2p2g_model(ctx, plan, m, ctx->d_halo_list, plan.counts_pending ? &ctx->d_halo_counts[0] : nullptr, ctx->n_halo, s);
	if(!plan.lean_events) {// (lean: the group loop records the event itself, once, behind its collect kernels)
		HIP_TRY(hipEventRecord(ctx->ev_halo, s));// the comm stream waits for this before collecting
		HIP_TRY(hipStreamWaitEvent(ctx->s_comm, ctx->ev_halo, 0));
	}
	guard.armed = false;
	return MPM_OK;
}
int mpm_g2p2g_halo(mpm_ctx* ctx, float dt, float next_dt) {
	phase_call(ctx);
	return ctx ? g2p2g_halo(ctx, default_plan(ctx, dt, next_dt)) : MPM_ERR_NOT_READY;
}

// plan.counts_pending: the host has not seen the counts of the tagging this launch runs on (the windowed group loop: the read-back of
// the previous substep is still outstanding).  n_inner is then one tagging old, and a rank whose interior block count has just left zero
// must not skip the launch - its interior blocks would be processed by neither pass and their particles would silently be gone.
// plan.ev.g2p2g_end marks the end.
static int g2p2g_interior(mpm_ctx* ctx, const SubstepPlan& plan) {
	if(!ctx || !ctx->ready || !ctx->halo_tagged) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
#if defined(MPM_EXPERIMENT) && defined(MPM_HACK_STALE_INTERIOR)// test only: round 4's bug - the launch is skipped on a count that is one tagging old (tests/test_mgsp_gpu.py shows that the library's books catch it)
	if(ctx->n_inner)
#else
	if(ctx->n_inner || plan.counts_pending)// all particle blocks in their own order, the halo ones skipped by flag (the block count is read from the status block)
#endif
		for(auto& m: ctx->models) launch_g2p2g_model(ctx, plan, m, nullptr, &ctx->d_status[ST_PBC], ctx->pbc, s, ctx->d_inner_list);
	HIP_TRY(hipEventRecord(plan.ev.g2p2g_end, s));
	HIP_TRY(hipGetLastError());
	return MPM_OK;
}
int mpm_g2p2g_interior(mpm_ctx* ctx, float dt, float next_dt) {
	phase_call(ctx);
	return ctx ? g2p2g_interior(ctx, default_plan(ctx, dt, next_dt)) : MPM_ERR_NOT_READY;
}

// the blocks shared with peers [peer0, peer0 + npeers) from grid gid on stream s, sizes from device memory (halo_collect_kernel);
// est_blocks: the host's estimate of the largest send count (launch size).  one_keys / one_blocks: see the kernel.
static int halo_collect(mpm_ctx* ctx, hipStream_t s, int gid, int peer0, int npeers, int rank, int est_blocks, float* out, size_t out_cap_floats, int* one_keys = nullptr, float* one_blocks = nullptr) {
	if(!ctx || !ctx->ready || !ctx->halo_tagged || peer0 < 0 || npeers < 1 || peer0 + npeers > 32 || gid < 0 || gid > 1) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	PeerSendLists ids;
	int rc = halo_send_lists(ctx, &ids, peer0, npeers, rank);
	if(rc) return rc;
	const unsigned nx = std::max(16u, std::min(4096u, cdiv((size_t) est_blocks + est_blocks / 4 + 64, 4)));
	halo_collect_kernel<<<dim3(nx, npeers), 256, 0, s>>>(&ctx->d_halo_counts[2], peer0, rank, ids, ctx->part[ctx->rollid].keys, ctx->grid[gid], out, out_cap_floats, one_keys, one_blocks);
	HIP_TRY(hipGetLastError());
	return MPM_OK;
}
int mpm_halo_collect(mpm_ctx* ctx, int peer, int gid, int* dev_keys, float* dev_blocks, int capacity_blocks, int* nsend) {
	phase_call(ctx);
	if(!ctx || !ctx->ready || !ctx->halo_tagged || peer < 0 || peer >= 32 || gid < 0 || gid > 1) return MPM_ERR_INVALID;
	const int n = ctx->send_count[peer];
	if(nsend) *nsend = n;
	if(n == 0) return MPM_OK;
	if(n > capacity_blocks) return fail(ctx, MPM_ERR_CAPACITY, "halo send buffer too small");
	return halo_collect(ctx, ctx->s_comm, gid, peer, 1, -1, n, nullptr, kHaloRow * (size_t) capacity_blocks, dev_keys, dev_blocks);
}

int mpm_halo_reduce(mpm_ctx* ctx, int gid, const int* dev_keys, const float* dev_blocks, int nrecv) {
	phase_call(ctx);
	if(!ctx || !ctx->ready || gid < 0 || gid > 1) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	if(nrecv > 0) halo_reduce_kernel<<<cdiv(nrecv, 4), 256, 0, ctx->s_comm>>>(ctx->g, nrecv, dev_keys, dev_blocks, ctx->part[ctx->rollid].table, ctx->nbc, ctx->grid[gid]);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(ctx->ev_comm, ctx->s_comm));
	HIP_TRY(hipStreamWaitEvent(ctx->s_compute, ctx->ev_comm, 0));// rebuild / grid update must see the summed blocks
	return MPM_OK;
}

// Debug read-out of the last tagging (tests/test_halo_kernels_gpu.py): the marks of the current partition's neighbour blocks, the halo
// list and the interior flags of its particle blocks, as the kernels left them.  Read-only; waits for both streams.
int mpm_halo_dump(mpm_ctx* ctx, int* overlap, int* halo_list, int* n_halo, int* inner_flags) {
	if(!ctx || !ctx->ready || !ctx->halo_tagged || !ctx->d_overlap) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipStreamSynchronize(ctx->s_compute));
	HIP_TRY(hipStreamSynchronize(ctx->s_comm));
	if(overlap && ctx->nbc) HIP_TRY(hipMemcpy(overlap, ctx->d_overlap, sizeof(int) * (size_t) ctx->nbc, hipMemcpyDeviceToHost));
	if(halo_list && ctx->n_halo) HIP_TRY(hipMemcpy(halo_list, ctx->d_halo_list, sizeof(int) * (size_t) ctx->n_halo, hipMemcpyDeviceToHost));
	if(inner_flags && ctx->pbc) HIP_TRY(hipMemcpy(inner_flags, ctx->d_inner_list, sizeof(int) * (size_t) ctx->pbc, hipMemcpyDeviceToHost));
	if(n_halo) *n_halo = ctx->n_halo;
	return MPM_OK;
}

// ---- fused substep (one host synchronisation) ----------------------------------------------------------------
static int mgsp_begin(mpm_ctx* ctx, const SubstepPlan& plan) {
	if(!ctx || !ctx->ready || !ctx->halo_tagged) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	if(!plan.lean_events) HIP_TRY(hipEventRecord(plan.ev.start, ctx->s_compute));
	int rc = launch_grid_update(ctx, plan.dt);
	if(rc) return rc;
	rc = halo_alloc(ctx);
	if(rc) return rc;
	return g2p2g_halo(ctx, plan);
}
static SubstepPlan mgsp_plan(const mpm_ctx* ctx, float dt, float next_dt) {// a fused substep that knows nothing about the next one (mpm_mgsp_begin, mpm_group_substep)
	SubstepPlan plan   = default_plan(ctx, dt, next_dt);
	plan.rebuild_clear = true;
	return plan;
}
int mpm_mgsp_begin(mpm_ctx* ctx, float dt, float next_dt) {
	phase_call(ctx);
	return ctx ? mgsp_begin(ctx, mgsp_plan(ctx, dt, next_dt)) : MPM_ERR_NOT_READY;
}

// tail != null: the rebuild's last kernel is left to the caller (launch_rebuild_prepare with *tail), see grp_substep_tail
static int mgsp_rebuild_export(mpm_ctx* ctx, const SubstepPlan& plan, int* dev_keys, int pad_rows, StillLaunch* tail) {
	if(!ctx || !ctx->ready || !dev_keys || pad_rows < 2) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	int rc = halo_alloc(ctx);
	if(rc) return rc;
	rc = launch_rebuild(ctx, plan, tail);
	if(rc) return rc;
	// the partition just rebuilt (it becomes current at mpm_mgsp_end); the export also resets the overlap marks and halo counters for
	// the tagging that follows, and puts this rank's status word into row 0
	return halo_export(ctx, ctx->rollid ^ 1, dev_keys, pad_rows);
}

int mpm_mgsp_rebuild_export(mpm_ctx* ctx, int* dev_keys, int pad_rows) {
	phase_call(ctx);
	return mgsp_rebuild_export(ctx, SubstepPlan {}, dev_keys, pad_rows, nullptr);
}

// on: the stream the two tagging kernels run on (the compute stream, or - group loop - the comm stream beside the rebuild's last kernel);
// plan.ev.end is recorded there when the tagging runs on the compute stream (the caller records it otherwise)
static int mgsp_tag(mpm_ctx* ctx, const SubstepPlan& plan, const int* dev_all_keys, int pad_rows, int world, int rank, hipStream_t on = nullptr) {
	if(!ctx || !ctx->ready || !dev_all_keys || world < 1 || world > 32) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	int rc = halo_alloc(ctx);
	if(rc) return rc;
	hipStream_t s = on ? on : ctx->s_compute;
	// (the overlap marks and the halo counters were cleared by the key export, which precedes this call in mpm_mgsp_rebuild_export)
	rc = halo_tag(ctx, ctx->rollid ^ 1, dev_all_keys, pad_rows, world, rank, s);
	if(rc) return rc;
	// (counts, peer list lengths / status words and the max |v|^2 slots come back with the status block at mpm_mgsp_end)
	if(!on && !plan.lean_events) HIP_TRY(hipEventRecord(plan.ev.end, s));// (lean: the read-back's event is the substep's end)
	ctx->mgsp_world = world;
	ctx->mgsp_rank	= rank;
	return MPM_OK;
}
int mpm_mgsp_tag(mpm_ctx* ctx, const int* dev_all_keys, int pad_rows, int world, int rank) {
	phase_call(ctx);
	if(ctx && ctx->body_mask) return fail(ctx, MPM_ERR_INVALID, "mpm_mgsp_tag: the context has a rigid body (mpm_set_collider_body); bodies in multi-GPU groups are not computed");
	if(ctx && ctx->force.count) return fail(ctx, MPM_ERR_INVALID, "mpm_mgsp_tag: the context has a force field (mpm_set_force_field); force fields in multi-GPU groups are not computed");
	return ctx ? mgsp_tag(ctx, default_plan(ctx), dev_all_keys, pad_rows, world, rank) : MPM_ERR_INVALID;
}

// The end of a fused substep in two halves: mgsp_end_enqueue rolls the partitions (host bookkeeping) and enqueues the read-back of the
// status block behind everything the substep has enqueued; mgsp_end_wait waits for it and takes the counts over.  mpm_mgsp_end does
// both at once; the windowed loop of mpm_group_run_fixed enqueues the next substep's grid update and halo-first G2P2G in between.
// plan.lean_events: plan.ev.end, the substep's timed end event, is recorded behind the read-back in place of ev_status
static int mgsp_end_enqueue(mpm_ctx* ctx, const SubstepPlan& plan) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	roll_partition(ctx);
	HIP_TRY(hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(int) * kStatusBlock, hipMemcpyDeviceToHost, ctx->s_compute));
	ctx->ev_pending = plan.lean_events ? plan.ev.end : ctx->ev_status;
	HIP_TRY(hipEventRecord(ctx->ev_pending, ctx->s_compute));
	return MPM_OK;
}
// the peers' status words of the last tagging (row 0 of their key lists): an error of ANY rank is every rank's error, in the same substep
static int mgsp_peer_status(mpm_ctx* ctx, int rank) {
	for(int p = 0; p < ctx->mgsp_world; ++p) {
		const int w = ctx->h_peer_rows[32 + p];
		if(p == rank || w == 0) continue;
		const std::string who = "rank " + std::to_string(p) + " reported: ";
		if(w & kPeerErrNonfinite) return fail(ctx, MPM_ERR_NONFINITE, who + "Maximum velocity is infinity");
		if(w & kPeerErrBlocks) return fail(ctx, MPM_ERR_CAPACITY, who + "block capacity exceeded");
		if(w & kPeerErrList) return fail(ctx, MPM_ERR_CAPACITY, who + "particles-per-block capacity exceeded");
		if(w & kPeerErrBins) return fail(ctx, MPM_ERR_CAPACITY, who + "bin capacity exceeded");
		if(w & kPeerErrBooks) return fail(ctx, MPM_ERR_INTERNAL, who + "particle books do not balance (bucketed + lost + dropped != added)");
		return fail(ctx, MPM_ERR_DEVICE, who + "status " + std::to_string(w));
	}
	return MPM_OK;
}
// ev: the substep's events; ev.start is the event its time is measured from
static int mgsp_end_wait(mpm_ctx* ctx, int rank, int* send_counts, int* halo_particle_blocks, int* max_peer_rows, float* max_vel_sqr, const SubstepEvents& ev) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	{// (short spin in front of the blocking wait, like sync_stream)
		const auto t0 = std::chrono::steady_clock::now();
		hipError_t q  = hipErrorNotReady;
		hipEvent_t done = ctx->ev_pending ? ctx->ev_pending : ctx->ev_status;
		while((q = hipEventQuery(done)) == hipErrorNotReady && std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(400)) {}
		if(q == hipErrorNotReady) q = hipEventSynchronize(done);
		HIP_TRY(q);
	}
	int rc = apply_status(ctx, nullptr);// this rank's own errors first, then its peers'
	if(rc) return rc;
	if(rank >= 0 && (rc = mgsp_peer_status(ctx, rank))) return rc;
	halo_take_counts(ctx);
	if(send_counts)
		for(int p = 0; p < 32; ++p) send_counts[p] = ctx->send_count[p];
	if(halo_particle_blocks) *halo_particle_blocks = ctx->n_halo;
	int mx = 0;
	for(int p = 0; p < ctx->mgsp_world; ++p) mx = std::max(mx, ctx->h_peer_rows[p] + 1);
	if(max_peer_rows) *max_peer_rows = mx;
	if(max_vel_sqr) *max_vel_sqr = host_maxvel(ctx);
	float t = 0.f;
	if(hipEventElapsedTime(&t, ev.g2p2g_start, ev.g2p2g_end) == hipSuccess) ctx->last_g2p2g_ms = ctx->timers.g2p2g_ms = t;
	if(hipEventElapsedTime(&t, ev.start, ev.end) == hipSuccess) ctx->timers.total_ms = t;
	return MPM_OK;
}
int mpm_mgsp_end(mpm_ctx* ctx, int* send_counts, int* halo_particle_blocks, int* max_peer_rows, float* max_vel_sqr) {
	phase_call(ctx);
	if(!ctx) return MPM_ERR_NOT_READY;
	int rc = mgsp_end_enqueue(ctx, default_plan(ctx));
	if(rc) return rc;
	return mgsp_end_wait(ctx, ctx->mgsp_rank, send_counts, halo_particle_blocks, max_peer_rows, max_vel_sqr, ctx->ev);
}
}
