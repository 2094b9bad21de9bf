// mpm_checkpoint.inc — full-state checkpoint / restart (SURVEY section 8 row f4; absent in the reference, whose only
// output is the per-frame position dump).  Included by claymore_hip.hip inside its extern "C" block.
//
// The state of a run at a substep boundary is: both partitions (the current numbering and the previous one, which the
// next G2P2G uses to find the particles' source bins), the current grid, and per model the source bins, both bin-offset
// tables, the block sizes and the advection lists.  Everything is stored compactly (used prefixes only; list rows packed
// by size[]); dense tables are rebuilt from the key lists on load.  A checkpoint is loaded into a context that has the
// same configuration and models and has been through mpm_initial_setup (capacities grow as needed).  After a load the
// MGSP halo tags are stale: run the tagging calls again before the next halo G2P2G.

namespace {
struct CkptModel {
	int32_t material, nch, list_in, layout;// layout: 0 = sliced advection lists, kPairLayoutId = the pair layout (mpm_kernels.hpp) with its per-chunk pair counts (1: the same with plain 512-record chunks, refused)
	int64_t n, bincount, bincount_src, bucketed;
};
struct CkptHeader {
	uint64_t magic;// "MPMCKPT7" (7: per-model list layout - sliced, or dense pairs with the pair counts of every chunk; 6: positions in cell units; 5: the solid models carry b = F F^T - 32-B records + a row; 4: 48-B records + a row of log Jp per bin; 3: field-wise parameter hash; 2: sliced advection lists, particle records)
	int32_t domain_bits, max_ppc, nmodels, rollid;
	int32_t pbc, nbc, ebc, prev_count;
	uint64_t total_bytes;
	uint64_t param_hash;// FNV-1a over the physical parameters (ckpt_param_hash): a checkpoint only loads into the same physics
	int32_t prev_pbc;// particle blocks of the previous numbering: the source-bin offsets that are in use
	int32_t grid_velocity;// 1: the grid was saved after a grid update (it holds velocities, not momenta: mpm_retrieve_velocity refuses it); 0 otherwise (formerly padding, always 0)
	CkptModel models[8];
};
constexpr uint64_t kCkptMagic = 0x3754504b434d504dull;

struct CkptLayout {
	size_t cur_keys, prev_keys, grid, end;
	size_t size[8], row_of[8], binoff_src[8], binoff_dst[8], bins[8], lists[8], pairinfo[8];
};
static CkptLayout ckpt_layout(const CkptHeader& h) {
	CkptLayout L {};
	size_t o	= sizeof(CkptHeader);
	auto take	= [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~size_t(15); return at; };
	L.cur_keys	= take(sizeof(int) * 3 * (size_t) h.ebc);
	L.prev_keys = take(sizeof(int) * 3 * (size_t) h.prev_count);
	L.grid		= take(sizeof(float) * 256 * (size_t) h.nbc);
	for(int m = 0; m < h.nmodels; ++m) {
		L.size[m]		= take(sizeof(int) * ((size_t) h.ebc + 1));
		L.row_of[m]		= take(sizeof(int) * ((size_t) h.ebc + 1));
		L.binoff_src[m] = take(sizeof(int) * ((size_t) h.prev_count + 1));
		L.binoff_dst[m] = take(sizeof(int) * ((size_t) h.ebc + 1));
		L.bins[m]		= take(sizeof(float) * (size_t) h.models[m].bincount_src * h.models[m].nch * kBin);
		L.lists[m]		= take(sizeof(int) * (size_t) h.models[m].bucketed);
		L.pairinfo[m]	= take(h.models[m].layout ? sizeof(int) * (size_t) h.pbc * kPairChunks : 0);
	}
	L.end = o;
	return L;
}
// FNV-1a over the PHYSICS of a run, field by field (not over raw struct bytes: padding, reserved fields and run-time policies
// - capacities, growth, overflow policy, synchronisation interval - may differ between the saving and the loading context;
// -0.0 and 0.0 are the same parameter)
static uint64_t ckpt_param_hash(const mpm_ctx* ctx) {
	uint64_t x = 1469598103934665603ull;
	auto mix_u = [&](uint32_t v) {
		for(int i = 0; i < 4; ++i) x = (x ^ ((v >> (8 * i)) & 0xffu)) * 1099511628211ull;
	};
	auto mix_i = [&](int v) { mix_u((uint32_t) v); };
	auto mix_f = [&](float f) {
		if(f == 0.f) f = 0.f;
		uint32_t u;
		memcpy(&u, &f, 4);
		mix_u(u);
	};
	const mpm_config& c = ctx->cfg;
	mix_i(c.domain_bits);
	mix_i(c.max_ppc);
	mix_i(c.boundary_blocks);
	mix_f(c.gravity);
	mix_f(c.cfl);
	for(const Model& M: ctx->models) {
		const mpm_material_params& p = M.p;
		mix_i(M.material);
		// only what make_material_const / the model's stress function consume: a parameter the material ignores may differ
		mix_f(p.rho);
		mix_f(p.volume);
		if(M.material == MPM_J_FLUID) {
			for(float f: {p.bulk, p.gamma, p.viscosity}) mix_f(f);
		} else {
			mix_f(p.youngs_modulus);
			mix_f(p.poisson_ratio);
		}
		if(M.material == MPM_SAND) {
			for(float f: {p.cohesion, p.beta, p.yield_surface, p.log_jp0}) mix_f(f);
			mix_i(p.volume_correction);
		}
		if(M.material == MPM_NACC) {
			for(float f: {p.beta, p.xi, p.msqr, p.log_jp0}) mix_f(f);
			mix_i(p.hardening_on);
		}
	}
	return x;
}
static int ckpt_header(mpm_ctx* ctx, CkptHeader& h) {
	memset(&h, 0, sizeof(h));
	h.magic		  = kCkptMagic;
	h.domain_bits = ctx->cfg.domain_bits;
	h.max_ppc	  = ctx->cfg.max_ppc;
	h.nmodels	  = (int) ctx->models.size();
	h.rollid	  = ctx->rollid;
	h.pbc		  = ctx->pbc;
	h.nbc		  = ctx->nbc;
	h.ebc		  = ctx->ebc;
	h.prev_pbc	  = ctx->pbc_prev;
	h.grid_velocity = ctx->grid_momentum ? 0 : 1;
	HIP_TRY(hipMemcpy(&h.prev_count, ctx->part[ctx->rollid ^ 1].count, sizeof(int), hipMemcpyDeviceToHost));
	for(int m = 0; m < h.nmodels; ++m) {
		const Model& M = ctx->models[m];
		h.models[m]	   = CkptModel {M.material, M.nch, M.list_in, M.pair ? kPairLayoutId : 0, (int64_t) M.n, M.bincount, M.bincount_src, M.bucketed};
	}
	h.total_bytes = ckpt_layout(h).end;
	h.param_hash  = ckpt_param_hash(ctx);
	return MPM_OK;
}
}// namespace

int mpm_checkpoint_size(mpm_ctx* ctx, size_t* bytes) {
	if(!ctx || !ctx->ready || !bytes) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	CkptHeader h;
	int rc = ckpt_header(ctx, h);
	if(rc) return rc;
	*bytes = h.total_bytes;
	return MPM_OK;
}

int mpm_checkpoint_save(mpm_ctx* ctx, void* buf, size_t capacity, size_t* written) {
	if(!ctx || !ctx->ready || !buf) return MPM_ERR_NOT_READY;
	if(ctx->grid_preupdated) return fail(ctx, MPM_ERR_NOT_READY, "a run was interrupted between two substeps: the grid is not in its canonical state");
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	CkptHeader h;
	int rc = ckpt_header(ctx, h);
	if(rc) return rc;
	if(capacity < h.total_bytes) return fail(ctx, MPM_ERR_CAPACITY, "checkpoint buffer too small: " + std::to_string(h.total_bytes) + " bytes needed");
	const CkptLayout L = ckpt_layout(h);
	char* out		   = (char*) buf;
	memset(out, 0, sizeof(CkptHeader));
	memcpy(out, &h, sizeof(h));
	const int r = ctx->rollid, n = r ^ 1;
	HIP_TRY(hipMemcpy(out + L.cur_keys, ctx->part[r].keys, sizeof(int) * 3 * (size_t) h.ebc, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out + L.prev_keys, ctx->part[n].keys, sizeof(int) * 3 * (size_t) h.prev_count, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out + L.grid, ctx->grid[0], sizeof(float) * 256 * (size_t) h.nbc, hipMemcpyDeviceToHost));
	for(int mi = 0; mi < h.nmodels; ++mi) {
		Model& M = ctx->models[mi];
		HIP_TRY(hipMemcpy(out + L.size[mi], M.size, sizeof(int) * ((size_t) h.ebc + 1), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(out + L.row_of[mi], M.row_of, sizeof(int) * ((size_t) h.ebc + 1), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(out + L.binoff_src[mi], M.binoff[r], sizeof(int) * ((size_t) h.prev_count + 1), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(out + L.binoff_dst[mi], M.binoff[n], sizeof(int) * ((size_t) h.ebc + 1), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(out + L.bins[mi], M.bins[r], sizeof(float) * (size_t) M.bincount_src * M.nch * kBin, hipMemcpyDeviceToHost));
		// pack the advection-list rows: prefix of size[] on the host, gather on the device
		const int* hsize = (const int*) (out + L.size[mi]);
		std::vector<long long> off((size_t) h.pbc + 1, 0);
		for(int b = 0; b < h.pbc; ++b) off[b + 1] = off[b] + hsize[b];
		if(off[h.pbc] != M.bucketed) return fail(ctx, MPM_ERR_INVALID, "checkpoint: list sizes do not add up to the bucketed particle count");
		if(h.pbc && M.bucketed) {
			DevBuf<long long> d_off;
			DevBuf<int> d_packed, d_info;
			HIP_TRY(d_off.alloc((size_t) h.pbc + 1, ctx->s_compute));
			HIP_TRY(d_packed.alloc((size_t) M.bucketed, ctx->s_compute));
			HIP_TRY(hipMemcpy(d_off, off.data(), sizeof(long long) * ((size_t) h.pbc + 1), hipMemcpyHostToDevice));
			if(M.pair) HIP_TRY(d_info.alloc((size_t) h.pbc * kPairChunks, ctx->s_compute));
			pack_lists_kernel<<<h.pbc, 64, 0, ctx->s_compute>>>(ctx->g.ppb, M.size, M.row_of, d_off, M.list[M.list_in], d_packed, M.pair ? 1 : 0, M.pairinfo[0], d_info);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(ctx->s_compute));
			HIP_TRY(hipMemcpy(out + L.lists[mi], d_packed, sizeof(int) * (size_t) M.bucketed, hipMemcpyDeviceToHost));
			if(M.pair) HIP_TRY(hipMemcpy(out + L.pairinfo[mi], d_info, sizeof(int) * (size_t) h.pbc * kPairChunks, hipMemcpyDeviceToHost));
		}
	}
	if(written) *written = h.total_bytes;
	return MPM_OK;
}

int mpm_checkpoint_load(mpm_ctx* ctx, const void* buf, size_t bytes) {
	phase_call(ctx);
	if(!ctx || !ctx->ready || !buf) return MPM_ERR_NOT_READY;
	if(bytes < sizeof(CkptHeader)) return fail(ctx, MPM_ERR_INVALID, "checkpoint: truncated header");
	CkptHeader h;
	memcpy(&h, buf, sizeof(h));
	if(h.magic != kCkptMagic) return fail(ctx, MPM_ERR_INVALID, "checkpoint: bad magic");
	if(h.domain_bits != ctx->cfg.domain_bits || h.max_ppc != ctx->cfg.max_ppc || h.nmodels != (int) ctx->models.size()) return fail(ctx, MPM_ERR_INVALID, "checkpoint: configuration or model count differs from the context");
	for(int m = 0; m < h.nmodels; ++m)
		if(h.models[m].material != ctx->models[m].material || h.models[m].n != (int64_t) ctx->models[m].n || h.models[m].layout != (ctx->models[m].pair ? kPairLayoutId : 0))
			return fail(ctx, MPM_ERR_INVALID, "checkpoint: model " + std::to_string(m) + " differs from the context (material, particle count or list layout)");
	if(h.param_hash != ckpt_param_hash(ctx)) return fail(ctx, MPM_ERR_INVALID, "checkpoint: configuration or material parameters differ from the context");
	const long long table_blocks = 1ll << (3 * (ctx->cfg.domain_bits - 2));
	if(h.pbc < 0 || h.pbc > h.nbc || h.nbc > h.ebc || h.ebc > table_blocks || h.prev_count < 0 || h.prev_count > table_blocks || (h.rollid != 0 && h.rollid != 1) || (h.grid_velocity != 0 && h.grid_velocity != 1) || h.prev_pbc < 0 || h.prev_pbc > h.prev_count)
		return fail(ctx, MPM_ERR_INVALID, "checkpoint: inconsistent block counts");
	for(int m = 0; m < h.nmodels; ++m) {
		const CkptModel& cm = h.models[m];
		const int64_t maxbins = cm.n / kBin + (int64_t) std::max(h.ebc, h.prev_count) + 1;
		if(cm.nch != ctx->models[m].nch || (cm.list_in != 0 && cm.list_in != 1) || cm.bucketed < 0 || cm.bucketed > cm.n || cm.bincount < 0 || cm.bincount > maxbins || cm.bincount_src < 0 || cm.bincount_src > maxbins)
			return fail(ctx, MPM_ERR_INVALID, "checkpoint: model " + std::to_string(m) + " has inconsistent counts");
	}
	const CkptLayout L = ckpt_layout(h);
	if(bytes < L.end || h.total_bytes != L.end) return fail(ctx, MPM_ERR_INVALID, "checkpoint: truncated");
	const char* in = (const char*) buf;
	// Everything that a kernel will use as an index is validated here, BEFORE the context is touched: a rejected checkpoint leaves
	// the context as it was.
	std::vector<std::vector<long long>> offs((size_t) h.nmodels);
	{
		const int tag_shift = ctx->g.pid_bits + kKeyBits;
		for(int mi = 0; mi < h.nmodels; ++mi) {
			const CkptModel& cm = h.models[mi];
			const int* hsize	= (const int*) (in + L.size[mi]);
			std::vector<long long>& off = offs[mi];
			off.assign((size_t) h.pbc + 1, 0);
			for(int b = 0; b < h.pbc; ++b) {
				if(hsize[b] < 0 || hsize[b] > ctx->g.ppb) return fail(ctx, MPM_ERR_INVALID, "checkpoint: corrupt list sizes");
				off[b + 1] = off[b] + hsize[b];
			}
			if(off[h.pbc] != cm.bucketed) return fail(ctx, MPM_ERR_INVALID, "checkpoint: corrupt list sizes");
			const int* bsrc = (const int*) (in + L.binoff_src[mi]);
			const int* bdst = (const int*) (in + L.binoff_dst[mi]);
			for(int b = 0; b < h.prev_pbc; ++b)// (entries behind the previous particle blocks are stale and never looked up)
				if(bsrc[b] < 0 || bsrc[b] > cm.bincount_src) return fail(ctx, MPM_ERR_INVALID, "checkpoint: corrupt bin offsets");
			for(int b = 0; b < h.pbc; ++b)
				if(bdst[b] < 0 || (long long) bdst[b] + (hsize[b] + kBin - 1) / kBin > cm.bincount) return fail(ctx, MPM_ERR_INVALID, "checkpoint: corrupt bin offsets");
			const int* recs = (const int*) (in + L.lists[mi]);
			for(long long i = 0; i < cm.bucketed; ++i)
				if(((((unsigned) recs[i]) >> tag_shift) & 31u) > 26u) return fail(ctx, MPM_ERR_INVALID, "checkpoint: corrupt advection records");// (above the tag: the pair layout's arena bit)
			if(cm.layout) {// the pair counts shape G2P2G's iterations: 2 Pf <= records of the chunk
				const int* pinfo = (const int*) (in + L.pairinfo[mi]);
				for(int b = 0; b < h.pbc; ++b)
					for(int c = 0; c < pair_chunks(hsize[b]); ++c) {
						const int pf = pinfo[(size_t) b * kPairChunks + c], nrec = pair_chunk_records(hsize[b], c);
						if(pf < 0 || 2 * pf > nrec) return fail(ctx, MPM_ERR_INVALID, "checkpoint: corrupt pair counts");
					}
			}
		}
		// every record must point INTO the bins of its source block: the block's extent is the distance to the next larger offset
		// (bins are handed out without gaps), the source block comes from the previous numbering's keys
		{
			const int G = ctx->g.G;
			const int* ckeys = (const int*) (in + L.cur_keys);
			const int* pkeys = (const int*) (in + L.prev_keys);
			std::vector<int> ptable((size_t) G * G * G, -1);
			auto kidx = [&](int x, int y, int z) { return ((size_t) x << (2 * ctx->g.gbits)) | ((size_t) y << ctx->g.gbits) | (size_t) z; };
			for(int b = 0; b < h.prev_count; ++b) {
				if(pkeys[3 * b] < 0 || pkeys[3 * b] >= G || pkeys[3 * b + 1] < 0 || pkeys[3 * b + 1] >= G || pkeys[3 * b + 2] < 0 || pkeys[3 * b + 2] >= G) return fail(ctx, MPM_ERR_INVALID, "checkpoint: block key outside the domain");
				ptable[kidx(pkeys[3 * b], pkeys[3 * b + 1], pkeys[3 * b + 2])] = b;
			}
			for(int mi = 0; mi < h.nmodels; ++mi) {
				const CkptModel& cm = h.models[mi];
				const int* bsrc		= (const int*) (in + L.binoff_src[mi]);
				std::vector<int> order((size_t) h.prev_pbc), extent((size_t) h.prev_pbc, 0);
				for(int b = 0; b < h.prev_pbc; ++b) order[b] = b;
				std::sort(order.begin(), order.end(), [&](int a, int c) { return bsrc[a] < bsrc[c]; });
				for(int i = 0; i < h.prev_pbc; ++i) {
					int j = i + 1;
					while(j < h.prev_pbc && bsrc[order[j]] == bsrc[order[i]]) ++j;// (empty blocks share an offset)
					extent[order[i]] = (int) std::min<long long>((j < h.prev_pbc ? (long long) bsrc[order[j]] : cm.bincount_src) - bsrc[order[i]], ctx->cfg.max_ppc);
				}
				const int* recs = (const int*) (in + L.lists[mi]);
				const std::vector<long long>& off = offs[mi];
				for(int b = 0; b < h.pbc; ++b) {
					const int kx = ckeys[3 * b], ky = ckeys[3 * b + 1], kz = ckeys[3 * b + 2];
					if(kx < 0 || kx >= G || ky < 0 || ky >= G || kz < 0 || kz >= G) return fail(ctx, MPM_ERR_INVALID, "checkpoint: block key outside the domain");
					int src[27];
					for(int t = 0; t < 27; ++t) {
						const int x = kx + t / 9 - 1, y = ky + (t / 3) % 3 - 1, z = kz + t % 3 - 1;
						src[t]		= (x < 0 || x >= G || y < 0 || y >= G || z < 0 || z >= G) ? -1 : ptable[kidx(x, y, z)];
					}
					for(long long i = off[b]; i < off[b + 1]; ++i) {
						const unsigned rec = (unsigned) recs[i];
						const int sno	   = src[(rec >> tag_shift) & 31u];
						const int sp	   = (int) (rec & (unsigned) (ctx->g.ppb - 1));
						if(sno < 0 || sno >= h.prev_pbc || (sp >> 6) >= extent[sno]) return fail(ctx, MPM_ERR_INVALID, "checkpoint: an advection record points outside its source block");
					}
				}
			}
		}
		const int* keys[2]	= {(const int*) (in + L.cur_keys), (const int*) (in + L.prev_keys)};
		const int nkeys[2] = {h.ebc, h.prev_count};
		for(int k = 0; k < 2; ++k)
			for(long long i = 0; i < 3ll * nkeys[k]; ++i)
				if(keys[k][i] < 0 || keys[k][i] >= ctx->g.G) return fail(ctx, MPM_ERR_INVALID, "checkpoint: block key outside the domain");
	}
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	hipStream_t s = ctx->s_compute;
	// make room (block-indexed arrays need max(ebc, prev_count) + 1 entries, bins bincount_src)
	const int need = std::max(h.ebc, h.prev_count);
	if(need > ctx->g.cap) {
		if(!ctx->cfg.grow) return fail(ctx, MPM_ERR_CAPACITY, "checkpoint needs " + std::to_string(need) + " blocks, capacity is " + std::to_string(ctx->g.cap));
		const size_t table = (size_t) table_blocks;
		while((size_t) need > (size_t) ctx->g.cap) {// the steps the growth policy would take (grow_capacity), the bins following the block capacity
			const size_t ncap = std::min(table, (size_t) ctx->g.cap * 3 / 2 + 1);
			if(ncap <= (size_t) ctx->g.cap) return fail(ctx, MPM_ERR_CAPACITY, "checkpoint needs " + std::to_string(need) + " blocks, more than the domain holds");// (the capacity stops growing at the table size)
			if(int rc = reserve_blocks(ctx, ncap)) return rc;
			if(int rc = grow_bins(ctx)) return rc;
		}
	}
	for(int m = 0; m < h.nmodels; ++m) {
		Model& M = ctx->models[m];
		const size_t nb = std::max<size_t>((size_t) h.models[m].bincount_src, (size_t) h.models[m].bincount);
		if(nb > M.bin_cap) {
			HIP_TRY(size_bin_arrays(ctx, M, nb));
			M.bin_cap = nb;
		}
	}
	// (a run that failed between two substeps may have left these set: the restored grid is the canonical one)
	ctx->grid_preupdated = false;
	ctx->rebuild_cleared = false;
	ctx->grid_momentum	 = h.grid_velocity == 0;
	if(ctx->load_gauge) HIP_TRY(hipMemsetAsync(ctx->d_load_acc, 0, sizeof(double) * kLoadAccDoubles, s));// (the gauge is no part of a checkpoint: it starts over)
	ctx->rollid	   = h.rollid;
	ctx->pbc	   = h.pbc;
	ctx->nbc	   = h.nbc;
	ctx->ebc	   = h.ebc;
	const int r = ctx->rollid, n = r ^ 1;
	const size_t table = (size_t) ctx->g.G * ctx->g.G * ctx->g.G;
	HIP_TRY(hipMemcpy(ctx->part[r].keys, in + L.cur_keys, sizeof(int) * 3 * (size_t) h.ebc, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(ctx->part[n].keys, in + L.prev_keys, sizeof(int) * 3 * (size_t) h.prev_count, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(ctx->part[r].count, &h.ebc, sizeof(int), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(ctx->part[n].count, &h.prev_count, sizeof(int), hipMemcpyHostToDevice));
	for(int i = 0; i < 2; ++i) HIP_TRY(hipMemsetAsync(ctx->part[i].table, 0xff, sizeof(int) * table, s));
	if(h.ebc) table_from_keys_kernel<<<cdiv(h.ebc, 256), 256, 0, s>>>(ctx->g, h.ebc, ctx->part[r].keys, ctx->part[r].table);
	if(h.prev_count) table_from_keys_kernel<<<cdiv(h.prev_count, 256), 256, 0, s>>>(ctx->g, h.prev_count, ctx->part[n].keys, ctx->part[n].table);
	HIP_TRY(hipMemcpyAsync(ctx->grid[0], in + L.grid, sizeof(float) * 256 * (size_t) h.nbc, hipMemcpyHostToDevice, s));
	for(int mi = 0; mi < h.nmodels; ++mi) {
		Model& M   = ctx->models[mi];
		M.list_in  = h.models[mi].list_in;
		M.bincount = h.models[mi].bincount;
		M.bincount_src = h.models[mi].bincount_src;
		M.bucketed = h.models[mi].bucketed;
		HIP_TRY(hipMemsetAsync(M.size, 0, sizeof(int) * ((size_t) ctx->g.cap + 1), s));
		HIP_TRY(hipMemcpyAsync(M.size, in + L.size[mi], sizeof(int) * ((size_t) h.ebc + 1), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(M.binoff[r], in + L.binoff_src[mi], sizeof(int) * ((size_t) h.prev_count + 1), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(M.binoff[n], in + L.binoff_dst[mi], sizeof(int) * ((size_t) h.ebc + 1), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(M.bins[r], in + L.bins[mi], sizeof(float) * (size_t) M.bincount_src * M.nch * kBin, hipMemcpyHostToDevice, s));
		const std::vector<long long>& off = offs[mi];
		if(h.pbc && M.bucketed) {
			DevBuf<long long> d_off;
			DevBuf<int> d_packed, d_info;
			hipError_t e = d_off.alloc((size_t) h.pbc + 1, s);
			if(e == hipSuccess) e = d_packed.alloc((size_t) M.bucketed, s);
			if(e == hipSuccess) e = hipMemcpyAsync(d_off, off.data(), sizeof(long long) * ((size_t) h.pbc + 1), hipMemcpyHostToDevice, s);
			if(e == hipSuccess) e = hipMemcpyAsync(d_packed, in + L.lists[mi], sizeof(int) * (size_t) M.bucketed, hipMemcpyHostToDevice, s);
			if(e == hipSuccess && M.pair) e = d_info.alloc((size_t) h.pbc * kPairChunks, s);
			if(e == hipSuccess && M.pair) e = hipMemcpyAsync(d_info, in + L.pairinfo[mi], sizeof(int) * (size_t) h.pbc * kPairChunks, hipMemcpyHostToDevice, s);
			if(e == hipSuccess) {
				unpack_lists_kernel<<<h.pbc, 64, 0, s>>>(ctx->g.ppb, M.size, M.row_of, d_off, M.list[M.list_in], d_packed, M.pair ? 1 : 0, M.pairinfo[0], d_info);
				e = hipGetLastError();
			}
			if(e == hipSuccess) e = hipStreamSynchronize(s);
			if(e != hipSuccess) return fail(ctx, MPM_ERR_DEVICE, std::string("checkpoint: ") + hipGetErrorString(e));
		}
	}
	// the counts the kernels read from the status block; the error flags of whatever happened before the load are cleared (they
	// describe the abandoned state), the cumulative lost / discarded / dropped counters stay
	{
		HIP_TRY(hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(int) * ST_WORDS, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		int* st		= ctx->h_status;
		st[ST_PBC] = h.pbc, st[ST_NBC] = h.nbc, st[ST_EBC] = h.ebc, st[ST_PBCPREV] = h.prev_pbc;
		ctx->pbc_prev = h.prev_pbc;
		st[ST_CNT_P] = st[ST_CNT_N] = st[ST_CNT_E] = 0;
		st[ST_OVERFLOW] = st[ST_NONFINITE] = 0;
		for(int mi = 0; mi < kMaxModels; ++mi) {
			st[ST_BINS0 + mi]	 = mi < h.nmodels ? (int) h.models[mi].bincount : 0;
			st[ST_BINSPREV + mi] = mi < h.nmodels ? (int) h.models[mi].bincount_src : 0;
			st[ST_PART0 + mi]	 = mi < h.nmodels ? (int) h.models[mi].bucketed : 0;
		}
		{// the books of the loaded state (check_books): what it holds + this context's cumulative counters + bias = what was added
			long long added = 0, held = 0;
			for(int mi = 0; mi < h.nmodels; ++mi) added += (long long) h.models[mi].n, held += (long long) h.models[mi].bucketed;
			ctx->books_bias = added - held - ((long long) st[ST_LOST] + (long long) st[ST_DROPPED]);
		}
		HIP_TRY(hipMemcpyAsync(ctx->d_status, st, sizeof(int) * ST_WORDS, hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemsetAsync(ctx->d_maxvel, 0, sizeof(unsigned) * kMaxVelSlots * kMaxVelStride, s));
	}
	// the per-block look-up rows are derived data: rebuild them (the stored lists are already sorted)
	{
		int rc = launch_prepare(ctx, PrepareFor::CheckpointLoad);
		if(rc) return rc;
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	ctx->halo_tagged = false;
	ctx->relaid		 = true;
	ctx->ids_valid	 = false;// ids are not part of the buffer: mpm_particle_ids_load brings them back
	return MPM_OK;
}
