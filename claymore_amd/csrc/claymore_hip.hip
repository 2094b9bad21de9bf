// claymore_hip.hip — host side of libclaymore_hip.so: the C ABI of include/claymore_amd.h on top of the gfx950
// kernels in mpm_kernels.hpp.  One context = one HIP device, two streams (compute, comm), all buffers owned here.
// Replaces the launch/orchestration part of GmpmSimulator (Projects/GMPM/gmpm_simulator.cuh:283-781) and the thin
// CUDA wrapper it sits on (Library/MnSystem/Cuda/Cuda.h, Cuda.cu).  No CPU fallback: every path needs a GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/claymore_amd.h"
#include "mpm_kernels.hpp"
#include "mpm_readout.hpp"
#include "mpm_grid_field.hpp"
#include "mpm_grid_isosurface.hpp"
#include "mpm_collision_mesh.hpp"
#include "mpm_mesh_fill.hpp"
#include "mpm_particle_init.hpp"
#include "mpm_particle_ids.hpp"
#include "mpm_particle_emit.hpp"
#include "mpm_particle_remove.hpp"
#include "mpm_force_field.hpp"
#include "mpm_collider_loads.hpp"
#include "mpm_rigid_body.hpp"
#include "mpm_storage.hpp"

using namespace mpm;

namespace {
// ONE device block (and its pinned mirror) holds everything the host reads back at a synchronisation: the status words, the MGSP halo
// counters + the peers' key-list lengths, and the max |v|^2 slots - one device-to-host copy instead of three.
constexpr int kHaloWords	 = 128;// 2 + 32 send counts + 32 peer list lengths + 32 peer status words, padded
constexpr int kStatusCore  = ST_WORDS + kHaloWords + kMaxVelSlots * kMaxVelStride;// in 4-byte words
// ... and behind them the phase stamps of mpm_run_fixed (mpm_kernels.hpp): one row per substep of the longest window (sync_interval is clamped to 64) and the row
// that closes it, 64-bit values, so they come back with the same copy
constexpr int kStampRows   = 64 + 1;
constexpr int kStatusBlock = kStatusCore + kStampRows * kStampRow * 2;
static_assert(kStatusCore % 2 == 0, "the stamps are 8-byte values");

// OWNERSHIP: every device array below is a DevBuf (mpm_storage.hpp), freed with the struct that holds it; the two rosters behind mpm_ctx
// state the size of every array that follows the block or the bin capacity.
struct Partition {
	DevBuf<int> table, keys, count;
};

struct Model {
	int material = 0;
	int nch		 = 0;
	mpm_material_params p {};
	MaterialConst mc {};
	size_t n	 = 0;
	DevBuf<float> d_xyz;// initial particle array; also the staging buffer of retrieve
	float v0[3]	 = {0, 0, 0};
	// per-particle initial conditions (mpm_add_model_particles; mpm_particle_init.hpp): the caller's arrays in the order of d_xyz, null where not given,
	// released when mpm_initial_setup returns; or a velocity field v0 + G (x - pivot) (mpm_set_model_velocity_field), never both a field and a velocity / affine array
	DevBuf<float> d_init_velocity, d_init_affine, d_init_state, d_init_logjp;
	int init_state_f = 0;// d_init_state holds F (MPM_STATE_F), else b as mpm_retrieve_state returns it
	bool has_field	 = false;
	VelocityField field {};
	DevBuf<float> bins[2];
	DevBuf<int> ids[2];// tracked contexts only (mpm_track_particle_ids): one int32 per bin slot, rolled and regrown with bins[] (mpm_particle_ids.hpp)
	size_t bin_cap = 0;
	DevBuf<int> binoff[2];
	DevBuf<int> list[2];
	DevBuf<int> size;
	DevBuf<int> row_of;
	DevBuf<int> out_count;
	DevBuf<int> keep;// per block of the numbering G2P2G ran in: its particle count if every particle stayed with an unchanged sort key, else -1
	DevBuf<int> blockinfo;// [block][kInfoRow], written by prepare_blocks_kernel
	bool pair = false;// the lists are in the pair layout (mpm_kernels.hpp) and G2P2G carries two particles per lane (mpm_g2p2g_pair.hpp)
	DevBuf<int> pairinfo[2];// pair layout only, [block][kPairChunks]: [0] full pairs per chunk of a block's sorted list (written by the sort, read by G2P2G), [1] what G2P2G hands on to the next sort
	int64_t bincount = 0;
	int64_t bincount_src = 0;// bins in use in bins[rollid] (the source of the next g2p2g): the previous bincount
	int64_t bucketed = 0;// particles currently in the advection lists (device-counted at each rebuild)
	int64_t removed	 = 0;// particles mpm_remove_particles has taken out of this model so far (reporting only: the books carry them in books_bias)
	int list_in		 = 0;// which list buffer g2p2g reads next
};

// How one rebuild launches, as launch_rebuild resolves it for its kernels, the last one (launch_rebuild_prepare) included: the workgroups of its own
// prepare launch and of its two registration launches, 0 = the full size (still_launch_rule); still: they may take the still path (mpm_kernels.hpp)
struct StillLaunch {
	int prepare = 0, reg = 0, still = 0;
};

}// namespace

// the timing events of one substep: start, G2P2G start, G2P2G end, end
struct SubstepEvents {
	hipEvent_t start = nullptr, g2p2g_start = nullptr, g2p2g_end = nullptr, end = nullptr;
};

// What the launches of ONE substep are offered.  The driver that enqueues the substep fills it once, every launch_* / mgsp_* / grp_* function below it
// takes it by const reference: none of it lives on the context, so no call inherits another call's offer.  The public phase-level entries use the defaults.
struct SubstepPlan {
	float dt = 0.f, next_dt = 0.f;
	SubstepEvents ev;// the events to record (single context: null G2P2G events are not recorded - a stamped substep)
	float fuse_dt = 0.f;// > 0: the driver knows the next substep's dt - the rebuild's carry-over applies that grid update too (and this substep's clear resets the max |v|^2 slots for it)
	bool offer_still = false;// the rebuild may take the still path (mpm_kernels.hpp) if G2P2G has moved nobody to another block: mpm_run_fixed on a single context alone
	bool rebuild_clear = false;// the rebuild follows in the same substep and nobody looks at the old table in between: its clear rides on the G2P2G prologue
	bool counts_pending = false;// the read-back of the last tagging's counts is outstanding (the deferred group loop): the halo launches size themselves from device memory
	// the windowed group loop in its deferred order: a substep records three events on the compute stream instead of seven (an event between two kernels is a barrier packet
	// of its own, 5-6 us: profiles/r06_rank_alone_seq.txt) - no start event (it is timed from the previous one's end), the end event doubles as the read-back's, one halo event
	bool lean_events = false;
	// mpm_run_fixed alone: the substep's row of the stamp ring, which launch_clear, the first model's G2P2G launch and the compaction pass on; null: timed with events
	unsigned long long* stamp_row = nullptr;
};
// What a prepare_blocks_kernel launch is for (launch_prepare derives its buffers, its template argument and its options from this alone).
enum class PrepareFor { Setup, CheckpointLoad, Rebuild };

struct mpm_ctx {
	mpm_config cfg {};
	GridCfg g {};
	int device = 0;
	hipStream_t s_compute = nullptr, s_comm = nullptr;
	SubstepEvents ev;// (a group's windowed loop times its substeps with two sets of its own: mpm_group.inc)
	hipEvent_t ev_comm = nullptr, ev_halo = nullptr;
	hipEvent_t ev_tag0 = nullptr, ev_tag1 = nullptr;// group loop: key list exported (compute -> comm) / tagging complete (comm -> compute); created on first use
	hipEvent_t ev_pending = nullptr;// the event the outstanding read-back completes with (SubstepPlan::lean_events: the substep's own end event)
	hipEvent_t ev_status = nullptr;
	// grid[0] already holds the velocities of the coming substep (the rebuild's carry-over applied the grid update for this dt):
	// only inside mpm_run_fixed, never when a call returns
	bool grid_preupdated = false;
	// grid[0] holds the mass and momentum of the last P2G (set-up, an unfused carry-over, a checkpoint that says so) - what mpm_retrieve_velocity
	// reads; a grid update turns the momenta into velocities in place, and a fused carry-over leaves velocities too: false until the next plain rebuild
	bool grid_momentum = false;
	float preupdate_dt	 = 0.f;
	// Between two host synchronisations of mpm_run_fixed the block counts below are ESTIMATES (the values of the last
	// synchronisation): launches are sized by them with a margin, every kernel reads the true counts from the status block.
	// The data was (re-)laid on the host - initial set-up, a checkpoint load, a capacity growth - since the last rebuild: that rebuild is not offered
	// the still path (mpm_kernels.hpp), whatever G2P2G says.  Cleared by every rebuild.
	bool relaid = true;
	// The rebuild's part of substep_clear_kernel has been issued together with the P2G part: the next rebuild's own clear skips it.  State of the device
	// data, not of a call: it must survive between the public calls mpm_mgsp_begin and mpm_mgsp_rebuild_export, which the Python MGSP driver issues separately.
	bool rebuild_cleared = false;
	// mpm_run_fixed's phase times come from stamps the kernels write (mpm_kernels.hpp: phase_stamp) unless MPM_PHASE_TIMERS=events asks for the HIP events of
	// old on every substep (read once, at creation: the A/B reference and the tests' comparison).
	bool phase_events = false;
	int wall_clock_khz = 0;
	unsigned long long* d_stamps = nullptr;// kStampRows rows of kStampRow, behind the max |v|^2 slots of the status block
	const unsigned long long* h_stamps = nullptr;
	// MPM_STILL_LAUNCH (read at creation; still_launch_rule): -1 auto, 0 full, N > 0 always thin with N workgroups.  streak_seen: ST_STREAK at the last read-back
	int still_launch = -1;
	int streak_seen	 = 0;
	std::vector<hipEvent_t> ev_ring;// 3 events per substep of a window (substep start, G2P2G start / end; its end is the next one's start) + the window's closing event
	Partition part[2];
	DevBuf<float> grid[2];
	int rollid	   = 0;
	int pbc = 0, nbc = 0, ebc = 0;
	int pbc_prev = 0;// particle blocks of the previous numbering (the one the particle data is laid out in)
	std::vector<Model> models;
	DevBuf<int> d_status;// kStatusBlock ints; the d_ / h_ pointers into it and into its pinned mirror (halo counts, peer rows, max |v|^2, stamps) are VIEWS, set once at set-up
	PinnedBuf<int> h_status;
	unsigned* d_maxvel = nullptr;
	float* h_maxvel	   = nullptr;
	DevBuf<double> d_totals;
	DevBuf<unsigned long long> d_counter;
	bool ready = false;
	int capacity_events = 0;// number of capacity growths so far (check_capacity)
	bool track_ids = false;// mpm_track_particle_ids: every model carries ids[2], moved beside every G2P2G launch
	bool ids_valid = false;// ids[rollid] names the particles of bins[rollid] (false between mpm_checkpoint_load and mpm_particle_ids_load)
	long long books_bias = 0;// check_books: particles a loaded checkpoint's state lacked beyond this context's own lost / dropped counters
	bool has_collision = false;// level-set collision object of the MGSP grid update
	CollisionObject collision {};// (collision.time is the clock: the time of the next grid update)
	bool collision_running = false;// the clock advances by dt with every grid update (mpm_set_collision_clock)
	DevBuf<float4> d_sdf;
	// analytic collision shapes (mpm_set_collision_shape): slot s is in use where shape[s].shape.kind != 0; they share the one clock above
	ShapeSlot shape[kMaxShapes] {};
	int shape_count = 0;// highest slot in use + 1
	// heightfields (mpm_set_collision_heightfield): slot s holds one where shape[s].shape.kind == kShapeHeightfield; hf[s].table is a view of
	// slot_table[s], which the context owns (a slot holds at most one of heightfield or volume).  hf_count > 0 selects the terrain kernels.
	DevBuf<float4> slot_table[kMaxShapes];
	Heightfield hf[kMaxShapes] {};
	int hf_count = 0;// slots that hold a heightfield
	// volumes (mpm_set_collision_volume, mpm_set_collision_volume_mesh): slot s holds one where shape[s].shape.kind == kShapeVolume; vol[s].table is
	// a view of slot_table[s] like a heightfield's; vol_desc[s] is the descriptor as installed (mpm_get_collision_volume).  vol_count > 0 selects
	// the volume kernels.
	Volume vol[kMaxShapes] {};
	mpm_collision_volume vol_desc[kMaxShapes] {};
	int vol_count = 0;// slots that hold a volume
	mpm_timers timers {};
	float last_g2p2g_ms = 0.f;
	// halo state (MGSP)
	DevBuf<int> d_overlap;// per neighbour block: bit mask of peers that also own it
	DevBuf<int> d_halo_list;// particle blocks touching an overlap block
	DevBuf<int> d_inner_list;// per particle block: 1 = interior (not touched by the halo-first pass)
	int* d_halo_counts = nullptr;// [0]=halo blocks, [1]=interior blocks, [2+peer]=send count for peer
	int* h_halo_counts = nullptr;// pinned mirror
	int* d_peer_rows   = nullptr;// key-list lengths exported by every rank (fused substep); lives behind d_halo_counts
	int* h_peer_rows   = nullptr;// pinned, behind h_halo_counts
	int mgsp_world	   = 0;
	int mgsp_rank	   = -1;// this rank's number in the last fused tagging (-1: none yet)
	bool halo_tagged   = false;
	// grid[0] holds the mass and momentum summed over the group's ranks on every node this rank's particles reach: set by a group call
	// that completed (mpm_group.inc), cleared at the start of every group call and by every phase-level call (phase_call)
	bool group_summed  = false;
	// the load gauge (mpm_load_gauge; mpm_collider_loads.hpp): on, launch_grid_update adds every stand-alone update's loads to d_load_acc first and
	// mpm_run_fixed keeps the update out of the carry-over.  Both arrays exist only while it is on.
	bool load_gauge = false;
	mpm_load_options load_opt {};
	DevBuf<double> d_load_partials;// kLoadGroups x [kLoadRows][kLoadSums]
	DevBuf<double> d_load_acc;// kLoadAccDoubles
	// rigid bodies (mpm_set_collider_body; mpm_rigid_body.hpp): bit s of body_mask = slot s is a body, its state, constants and float32 pose live in
	// d_body (allocated at the first install, with the partials of grid_update_body_kernel); body_c / body_desc are the host's copies of the constants.
	// frozen: slot s was a body and is prescribed again, at rest at frozen_pose[s] (until the next install over the slot)
	int body_mask = 0;
	DevBuf<BodyBlock> d_body;
	DevBuf<double> d_body_partials;// kLoadGroups x [kLoadRows][kLoadSums]
	BodyConst body_c[kMaxBodies] {};
	mpm_rigid_body body_desc[kMaxBodies] {};
	bool frozen[kMaxBodies] = {};
	CollisionPose frozen_pose[kMaxBodies] {};
	// force fields (mpm_set_force_field; mpm_force_field.hpp): the slots as the kernels read them, by value - nothing on the device.  force.count > 0:
	// launch_grid_update runs grid_force_kernel ahead of every applied update and mpm_run_fixed keeps the update out of the carry-over.
	ForceArgs force {};
	int group_refs	   = 0;// mpm_group handles on this context (grp_common_init / mpm_group_destroy): the single-context readouts refuse it
	DevBuf<int> d_send_ids[32];
	int n_halo = 0, n_inner = 0;
	int send_count[32] = {0};
	std::string err;
};

// THE TWO ROSTERS: every array whose size follows the block capacity - f(buf, elements per block, extra elements) - or a model's bin capacity -
// f(buf, elements per bin) -, each size stated once.  Set-up, growth, a checkpoint load and the halo arrays' first use all size by them: a new
// per-block array is one line here.  lazy: the halo arrays too, which halo_alloc / halo_send_lists allocate on first use (null until then).
template<class F>
static void for_block_arrays(mpm_ctx* ctx, bool lazy, F&& f) {
	for(int i = 0; i < 2; ++i) f(ctx->part[i].keys, 3, 0), f(ctx->grid[i], 256, 0);
	for(auto& m: ctx->models) {
		for(int i = 0; i < 2; ++i) f(m.binoff[i], 1, 1), f(m.list[i], ctx->g.ppb, 0);
		f(m.size, 1, 1), f(m.row_of, 1, 1), f(m.out_count, 1, 1), f(m.keep, 1, 1);
		f(m.blockinfo, kInfoRow, 0);
		if(m.pair)
			for(int i = 0; i < 2; ++i) f(m.pairinfo[i], kPairChunks, kPairChunks);
	}
	if(!lazy) return;
	f(ctx->d_overlap, 1, 1), f(ctx->d_halo_list, 1, 1), f(ctx->d_inner_list, 1, 1);
	for(auto& ids: ctx->d_send_ids) f(ids, 1, 1);
}
template<class F>
static void for_bin_arrays(mpm_ctx* ctx, Model& m, F&& f) {
	for(int i = 0; i < 2; ++i) {
		f(m.bins[i], m.nch * kBin);
		if(ctx->track_ids) f(m.ids[i], kBin);
	}
}
// Every block array (lazy: and every halo array that exists) to at least ncap blocks, every bin array of m to at least nb bins; an array that does
// not exist yet is allocated.  A failure half-way leaves every array at least as large as it was.
static hipError_t size_block_arrays(mpm_ctx* ctx, size_t ncap, bool lazy) {
	hipError_t e = hipSuccess;
	for_block_arrays(ctx, lazy, [&](auto& buf, size_t per, size_t extra) {
		if(e == hipSuccess && (buf.p || !lazy)) e = buf.grow(ncap * per + extra, ctx->s_compute);
	});
	return e;
}
static hipError_t size_bin_arrays(mpm_ctx* ctx, Model& m, size_t nb) {
	hipError_t e = hipSuccess;
	for_bin_arrays(ctx, m, [&](auto& buf, size_t per) {
		if(e == hipSuccess) e = buf.grow(nb * per, ctx->s_compute);
	});
	return e;
}
// A lazily allocated array of the block roster comes to life at the present capacity, with the size its roster line states.
template<class B>
static hipError_t alloc_block_array(mpm_ctx* ctx, B& want) {
	hipError_t e = hipSuccess;
	for_block_arrays(ctx, true, [&](auto& buf, size_t per, size_t extra) {
		if((void*) &buf == (void*) &want) e = buf.alloc((size_t) ctx->g.cap * per + extra, ctx->s_compute);
	});
	return e;
}

// The plan of a public phase-level entry, and what every driver starts from: the context's own events, nothing offered.
static SubstepPlan default_plan(const mpm_ctx* ctx, float dt = 0.f, float next_dt = 0.f) {
	return {dt, next_dt, ctx->ev};
}

// An interrupted call leaves no promise about the grid behind (a checkpoint load restores a canonical one): the two flags that span
// kernels - grid already updated for the next dt, rebuild clear already issued - are reset on EVERY error exit (HIP_TRY returns included), by scope.
struct FlagGuard {
	mpm_ctx* ctx;
	bool armed = true;
	~FlagGuard() {
		if(armed) ctx->grid_preupdated = ctx->rebuild_cleared = false;
	}
};

#define HIP_TRY(expr)                                                                                            \
	do {                                                                                                         \
		hipError_t e_ = (expr);                                                                                  \
		if(e_ != hipSuccess) {                                                                                   \
			ctx->err = std::string(#expr) + " -> " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"; \
			return MPM_ERR_DEVICE;                                                                               \
		}                                                                                                        \
	} while(0)

// the grid update leaves its running maximum in kMaxVelSlots slots (non-negative floats; inf marks a NaN velocity)
static float host_maxvel(const mpm_ctx* ctx) {
	float m = 0.f;
	for(int i = 0; i < kMaxVelSlots; ++i) m = std::max(m, ctx->h_maxvel[i * kMaxVelStride]);
	return m;
}

// Which materials' G2P2G runs two particles per lane (bit m = material m; mpm_g2p2g_pair.hpp).
// MPM_PAIR_DEFAULT: the ones used unless the environment says otherwise (MPM_G2P2G_PAIRS=<mask>, read once: same-library A/B and tests).
#ifndef MPM_PAIR_DEFAULT
#define MPM_PAIR_DEFAULT 0xF// all four materials (NACC with the late record fetch: 163 registers, no scratch; -6 % on a 5 M-particle NACC sphere)
#endif
static int pair_mask() {
	static const int mask = [] {
		const char* e = std::getenv("MPM_G2P2G_PAIRS");
		return (e && *e ? (int) std::strtol(e, nullptr, 0) : MPM_PAIR_DEFAULT) & 0xF;
	}();
	return mask;
}

// two particles per lane (mpm_g2p2g_pair.hpp) for the materials of pair_mask(); the others one particle per lane (same signature)
template<int M>
static auto g2p2g_for(bool pair) {
	return pair ? g2p2g_pair_kernel<M> : g2p2g_kernel<M>;
}

static int launch_prepare(mpm_ctx* ctx, PrepareFor why, const StillLaunch& thin = {});

static int fail(mpm_ctx* ctx, int code, const std::string& msg) {
	ctx->err = msg;
	return code;
}

// Every public phase-level entry (a grid update, a G2P2G pass, a rebuild, the halo / MGSP phases, a checkpoint load, the single-context
// substep drivers) calls this first: from then on a grouped context's grid[0] is no longer known to hold the group's summed momentum,
// until the next group call that completes (mpm_group_retrieve_velocity).
static inline void phase_call(mpm_ctx* ctx) {
	if(ctx) ctx->group_summed = false;
}

static inline unsigned cdiv(size_t a, size_t b) {
	return (unsigned) ((a + b - 1) / b);
}

// LAUNCH SIZES THAT FOLLOW THE STILL STREAK.  From the second still rebuild in a row on, prepare_blocks_kernel<true> looks at 64 blocks per wave and finds next
// to nothing to do; sized by the block estimate - one workgroup per exterior block, 89 000 at C3, of which 1 310 look at anything - its launch costs 24 us for
// work that fits into the 4.7 us a launch takes at the least.  The kernel walks grid-stride over a count it reads from the status block, so any launch size
// computes the same: when the streak was two or more at the last read-back (and the still path is on) the next window launches it THIN, with kThinPrepare
// workgroups - never fewer than one per 64 particle blocks (the streak path stays one trip), and enough to fill the chip's wave slots when a thin window
// meets a mover and runs the full path (six waves per SIMD: 6 144).  The next read-back then finds the streak at 0 and the launch goes back to full size.
// Measured at C3 (profiles/substep_fixed_cost.txt): 1 024, 4 096, 8 192 and 16 384 workgroups all run in 4.7 us, 256 in 7.9 us.  The two registration
// kernels, which return behind their first loads on a still substep, take those 4.7 us at their present 4 096 / 8 192 workgroups as at 256: they keep
// their sizes (the second number is for MPM_STILL_LAUNCH=thin:N alone).
// override_n (MPM_STILL_LAUNCH): -1 auto = this rule, 0 full = never thin, N > 0 always N workgroups for prepare and both registrations (tests and A/B only).
// Returns workgroup counts, 0 = the full size; the caller never launches more than the full size.
constexpr int kThinPrepare = 8192;
static StillLaunch still_launch_rule(int streak, bool still_on, int pbc_est, int override_n) {
	if(override_n > 0) return {override_n, override_n};
	if(override_n == 0 || !still_on || streak < 2) return {0, 0};
	const long long looked = (long long) std::max(pbc_est, 0) + std::max(pbc_est, 0) / 16 + 64;// (the margin of hint_blocks)
	return {(int) std::max<long long>(kThinPrepare, (looked + 63) / 64), 0};
}
// "auto" (or nothing, or anything else) -1, "full" 0, "thin:N" N >= 1
static int still_launch_override(const char* e) {
	if(!e) return -1;
	if(std::strcmp(e, "full") == 0) return 0;
	if(std::strncmp(e, "thin:", 5) == 0) {
		char* end	 = nullptr;
		const long n = std::strtol(e + 5, &end, 10);
		if(end != e + 5 && *end == 0 && n >= 1 && n <= (1 << 20)) return (int) n;
	}
	return -1;
}

// The installed colliders as the grid update that is being enqueued sees them, handed to `launch` in the type of their kernels: VolumeColliderArgs
// with a volume in a slot (BodyArgs around it with a rigid body in a slot), else TerrainArgs with a heightfield in a slot, ShapeArgs with analytic shapes alone, CollisionArgs with the level-set object alone, NoCollision without any.
// One pose per installed collider, all at the one clock's current time T (the start of the substep), by value; a running clock then moves
// on, T = T + dt in one float32 addition (the drivers' own cur_time += dt).  Called once per applied grid update - by the stand-alone
// kernel's launch or by the fused carry-over's, never by both.  state_pivots: BodyArgs' own, for the launches whose kernel sums loads.
template<class F>
static void with_collider(mpm_ctx* ctx, float dt, F&& launch, int state_pivots = 0) {
	if(!ctx->has_collision && !ctx->shape_count) {
		launch(NoCollision {});
		return;
	}
	const float T = ctx->collision.time;
	VolumeColliderArgs va {};
	TerrainArgs& a	= va.ter;
	a.col.count		= ctx->shape_count;
	a.col.has_field = ctx->has_collision ? 1 : 0;
	if(ctx->has_collision) a.col.field = CollisionArgs {ctx->collision, collision_pose(ctx->collision, T)};
	for(int i = 0; i < ctx->shape_count; ++i) {
		a.col.slot[i] = ctx->shape[i];
		if(a.col.slot[i].shape.kind) a.col.slot[i].pose = ctx->frozen[i] ? ctx->frozen_pose[i] : collision_pose(a.col.slot[i].obj, T);
	}
	for(int i = 0; i < kMaxShapes; ++i) a.hf[i] = ctx->hf[i], va.vol[i] = ctx->vol[i];
	if(ctx->collision_running) ctx->collision.time = T + dt;
	if(ctx->body_mask)// (a body slot's pose and pivot are read from the device; its object travels with trans = com and no velocity)
		launch(BodyArgs {va, ctx->d_body.p->pose, ctx->d_body.p->st, ctx->body_mask, state_pivots});
	else if(ctx->vol_count)
		launch(va);
	else if(ctx->hf_count)
		launch(a);
	else if(ctx->shape_count)
		launch(a.col);
	else
		launch(a.col.field);
}
// The installed colliders at the clock's current time T as with_collider hands them out, without its side effect: the clock stays where it is.
// What a readout of the coming grid update needs (mpm_collider_loads.hpp); the two launches that apply an update call with_collider itself.
template<class F>
static void with_collider_at_clock(mpm_ctx* ctx, F&& launch, int state_pivots = 0) {
	const float T = ctx->collision.time;
	with_collider(ctx, 0.f, launch, state_pivots);
	ctx->collision.time = T;
}

extern "C" {

int mpm_default_config(int domain_bits, mpm_config* cfg) {
	if(!cfg || domain_bits < 4 || domain_bits > 10) return MPM_ERR_INVALID;
	memset(cfg, 0, sizeof(*cfg));
	cfg->domain_bits	 = domain_bits;
	cfg->max_ppc		 = 128;	  // settings.h:75
	cfg->boundary_blocks = 2;	  // settings.h:63
	cfg->gravity		 = -9.8f; // settings.h:85
	cfg->cfl			 = 0.5f;  // settings.h:53
	cfg->max_blocks		 = 0;
	cfg->grow			 = 1;
	return MPM_OK;
}

int mpm_default_material(int material, int domain_bits, mpm_material_params* p) {
	if(!p) return MPM_ERR_INVALID;
	memset(p, 0, sizeof(*p));
	const float n	  = (float) (1u << domain_bits);
	p->rho			  = 1e3f;// settings.h:81-83
	p->youngs_modulus = 5e3f;
	p->poisson_ratio  = 0.4f;
	const float vol1  = 1.0f / n / n / n / 8.0f;
	const float vol10 = 10.f / n / n / n / 8.0f;// particle_buffer.cuh:176,:203 (sic)
	switch(material) {
		case MPM_J_FLUID:
			p->volume	 = vol1;
			p->bulk		 = 4e4f;
			p->gamma	 = 7.15f;
			p->viscosity = 0.01f;
			break;
		case MPM_FIXED_COROTATED: p->volume = vol10; break;
		case MPM_SAND:
			p->volume			 = vol10;
			p->cohesion			 = 0.f;
			p->beta				 = 1.f;
			p->yield_surface	 = 0.816496580927726f * 2.f * 0.5f / (3.f - 0.5f);
			p->volume_correction = 1;
			p->log_jp0			 = 0.f;
			break;
		case MPM_NACC:
			p->volume		= vol1;
			p->xi			= 0.8f;
			p->beta			= 0.5f;
			p->msqr			= 3.423772074299613f;
			p->hardening_on = 1;
			p->log_jp0		= -0.01f;
			break;
		default: return MPM_ERR_INVALID;
	}
	return MPM_OK;
}

static MaterialConst make_material_const(const mpm_material_params& p) {
	MaterialConst mc {};
	const float e = p.youngs_modulus, nu = p.poisson_ratio;
	mc.volume			 = p.volume;
	mc.mass				 = p.volume * p.rho;						  // particle_buffer.cuh:158,:186,:252
	mc.lambda			 = e * nu / ((1 + nu) * (1 - 2 * nu));		  // :187
	mc.mu				 = e / (2 * (1 + nu));						  // :188
	mc.bm				 = 2.f / 3.f * (e / (2 * (1 + nu))) + (e * nu / ((1 + nu) * (1 - 2 * nu)));// :255
	mc.bulk				 = p.bulk;
	mc.gamma			 = p.gamma;
	mc.viscosity		 = p.viscosity;
	mc.cohesion			 = p.cohesion;
	mc.beta				 = p.beta;
	mc.yield_surface	 = p.yield_surface;
	mc.xi				 = p.xi;
	mc.msqr				 = p.msqr;
	mc.log_jp0			 = p.log_jp0;
	mc.volume_correction = p.volume_correction;
	mc.hardening_on		 = p.hardening_on;
	return mc;
}

int mpm_create(const mpm_config* cfg, int device, mpm_ctx** out) {
	if(!cfg || !out) return MPM_ERR_INVALID;
	if(cfg->domain_bits < 4 || cfg->domain_bits > 10) return MPM_ERR_INVALID;
	if(cfg->max_ppc < 1 || cfg->max_ppc > 128 || (cfg->max_ppc & (cfg->max_ppc - 1))) return MPM_ERR_INVALID;
	int ndev = 0;
	if(hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || device < 0 || device >= ndev) {
		fprintf(stderr, "claymore_hip: no usable HIP device %d (found %d) - there is no CPU fallback\n", device, ndev);
		return MPM_ERR_DEVICE;
	}
	mpm_ctx* ctx = new mpm_ctx();
	ctx->cfg	 = *cfg;
	ctx->device	 = device;
	GridCfg& g	 = ctx->g;
	g.gbits		 = cfg->domain_bits - 2;
	g.G			 = 1 << g.gbits;
	g.ppb		 = cfg->max_ppc * 64;
	g.pid_bits	 = 0;
	while((1 << g.pid_bits) < g.ppb) g.pid_bits++;
	g.boundary = cfg->boundary_blocks;
	g.dx_inv   = (float) (1 << cfg->domain_bits);
	g.dx	   = 1.f / g.dx_inv;
	g.d_inv	   = 4.f * g.dx_inv * g.dx_inv;
	g.gravity  = cfg->gravity;
	g.cap	   = 0;
	// the comm stream gets the highest priority: its small collect / reduce kernels (and RCCL's) are enqueued BEHIND the big
	// interior G2P2G and must not wait for it to drain
	int prio_lo = 0, prio_hi = 0;
	if(hipSetDevice(device) == hipSuccess) hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
	if(hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->s_compute, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithPriority(&ctx->s_comm, hipStreamNonBlocking, prio_hi) != hipSuccess) {
		delete ctx;
		return MPM_ERR_DEVICE;
	}
	if(hipEventCreate(&ctx->ev.start) != hipSuccess || hipEventCreate(&ctx->ev.end) != hipSuccess || hipEventCreate(&ctx->ev.g2p2g_start) != hipSuccess || hipEventCreate(&ctx->ev.g2p2g_end) != hipSuccess
	   || hipEventCreateWithFlags(&ctx->ev_comm, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_halo, hipEventDisableTiming) != hipSuccess
	   || hipEventCreateWithFlags(&ctx->ev_status, hipEventDisableTiming) != hipSuccess) {
		mpm_destroy(ctx);// frees whatever was created (null handles are skipped)
		return MPM_ERR_DEVICE;
	}
	{
		const char* e = std::getenv("MPM_PHASE_TIMERS");
		ctx->phase_events = e && std::strcmp(e, "events") == 0;
		// (the stamps are ticks of the constant wall clock: a runtime that does not report its rate leaves the events)
		if(hipDeviceGetAttribute(&ctx->wall_clock_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || ctx->wall_clock_khz <= 0) ctx->phase_events = true;
		ctx->still_launch = still_launch_override(std::getenv("MPM_STILL_LAUNCH"));
	}
	*out = ctx;
	return MPM_OK;
}

void mpm_destroy(mpm_ctx* ctx) {
	if(!ctx) return;
	hipSetDevice(ctx->device);
	hipDeviceSynchronize();
	for(hipEvent_t e: {ctx->ev.start, ctx->ev.g2p2g_start, ctx->ev.g2p2g_end, ctx->ev.end})
		if(e) hipEventDestroy(e);
	if(ctx->ev_comm) hipEventDestroy(ctx->ev_comm);
	if(ctx->ev_halo) hipEventDestroy(ctx->ev_halo);
	if(ctx->ev_tag0) hipEventDestroy(ctx->ev_tag0);
	if(ctx->ev_tag1) hipEventDestroy(ctx->ev_tag1);
	if(ctx->ev_status) hipEventDestroy(ctx->ev_status);
	for(hipEvent_t e: ctx->ev_ring) hipEventDestroy(e);
	if(ctx->s_compute) hipStreamDestroy(ctx->s_compute);
	if(ctx->s_comm) hipStreamDestroy(ctx->s_comm);
	delete ctx;// (every device array goes with its owner: mpm_storage.hpp)
}

const char* mpm_last_error(const mpm_ctx* ctx) {
	return ctx ? ctx->err.c_str() : "null context";
}

// The view of a model's per-particle arrays that the set-up kernels take.
static ParticleInit particle_init_view(const Model& m) {
	ParticleInit a;
	a.velocity = m.d_init_velocity.n ? m.d_init_velocity.p : nullptr;
	a.affine9  = m.d_init_affine.n ? m.d_init_affine.p : nullptr;
	a.state9   = m.d_init_state.n ? m.d_init_state.p : nullptr;
	a.logjp	   = m.d_init_logjp.n ? m.d_init_logjp.p : nullptr;
	a.state_f  = m.init_state_f;
	return a;
}

// mpm_add_model_particles' arrays: copied into buffers the model owns, then checked on the device by one reduction kernel (the host walks no row).
static int stage_particle_init(mpm_ctx* ctx, Model& m, const mpm_particle_init* init) {
	const char* who = "mpm_add_model_particles";
	for(int r: init->reserved)
		if(r) return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": a reserved word of mpm_particle_init is not 0");
	const bool fluid = m.material == MPM_J_FLUID;
	if(init->state9 && init->state_kind != MPM_STATE_B && init->state_kind != MPM_STATE_F)
		return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": unknown state_kind " + std::to_string(init->state_kind) + " (MPM_STATE_B or MPM_STATE_F)");
	if(!m.n) return MPM_OK;// (an empty model carries nothing)
	hipStream_t s = ctx->s_compute;
	const bool with_logjp = init->logjp && (m.material == MPM_SAND || m.material == MPM_NACC);// (ignored where the material has no log Jp)
	struct {
		const float* host;
		DevBuf<float>* dev;
		size_t per;
	} cols[4] = {{init->velocity, &m.d_init_velocity, 3}, {init->affine9, &m.d_init_affine, 9}, {init->state9, &m.d_init_state, 9}, {with_logjp ? init->logjp : nullptr, &m.d_init_logjp, 1}};
	for(auto& c: cols) {
		if(!c.host) continue;
		if(c.dev->alloc(c.per * m.n, s) != hipSuccess) return fail(ctx, MPM_ERR_CAPACITY, std::string(who) + ": no device memory for the per-particle arrays");
		HIP_TRY(hipMemcpyAsync(c.dev->p, c.host, sizeof(float) * c.per * m.n, hipMemcpyHostToDevice, s));
	}
	m.init_state_f = init->state9 && init->state_kind == MPM_STATE_F ? 1 : 0;
	const ParticleInit a = particle_init_view(m);
	if(!a.velocity && !a.affine9 && !a.state9 && !a.logjp) return MPM_OK;
	DevBuf<int> flag;
	HIP_TRY(flag.alloc(1, s));
	validate_particle_init_kernel<<<std::min(4096u, cdiv(m.n, 256)), 256, 0, s>>>(m.n, fluid, a, flag.p);
	int bad = 0;
	HIP_TRY(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if(bad & kInitBadVelocity) return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": velocity holds a value that is not finite");
	if(bad & kInitBadAffine) return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": affine9 holds a value that is not finite");
	if(bad & kInitBadState) return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": state9 holds a value that is not finite");
	if(bad & kInitBadLogJp) return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": logjp holds a value that is not finite");
	if(bad & kInitNotPositive) return fail(ctx, MPM_ERR_INVALID, std::string(who) + (fluid ? ": state9 holds a J that is not strictly positive" : ": state9 holds a |b00|, b11 or b22 that is not strictly positive"));
	return MPM_OK;
}

static int add_model(mpm_ctx* ctx, const char* who_name, int material, const mpm_material_params* params, const float* xyz, size_t n, const float v0[3], const mpm_particle_init* init, int* model_id) {
	if(!ctx) return MPM_ERR_INVALID;
	const std::string who = who_name;
	if(!params) return fail(ctx, MPM_ERR_INVALID, who + ": material parameters are missing");
	if(ctx->ready) return fail(ctx, MPM_ERR_INVALID, who + ": models must be added before mpm_initial_setup");
	if(!xyz && n) return fail(ctx, MPM_ERR_INVALID, who + ": positions are missing");
	if(material < 0 || material > 3) return fail(ctx, MPM_ERR_INVALID, "unknown material");
	if((int) ctx->models.size() >= kMaxModels) return fail(ctx, MPM_ERR_CAPACITY, "too many models");
	HIP_TRY(hipSetDevice(ctx->device));
	Model m;
	m.material = material;
	m.p		   = *params;
	m.mc	   = make_material_const(*params);
	m.nch	   = material == MPM_J_FLUID ? 4 : (material == MPM_FIXED_COROTATED ? 9 : 10);// floats per particle in a bin (mpm_g2p2g.hpp: {x, y, z, J}, or a 32-B record {x, y, z, b...} + a row of b21 (+ log Jp))
	m.n		   = n;
	for(int d = 0; d < 3; ++d) m.v0[d] = v0 ? v0[d] : 0.f;
	HIP_TRY(m.d_xyz.alloc(3 * n, ctx->s_compute));
	if(n) {// an empty model is legal (an MGSP rank whose slab of a model is empty, an empty sampled SDF)
		HIP_TRY(hipMemcpyAsync(m.d_xyz, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, ctx->s_compute));
		HIP_TRY(hipStreamSynchronize(ctx->s_compute));
	}
	if(init)// (a refused call changes nothing: m goes with this scope)
		if(int rc = stage_particle_init(ctx, m, init)) return rc;
	if(model_id) *model_id = (int) ctx->models.size();
	ctx->models.push_back(std::move(m));
	return MPM_OK;
}

int mpm_add_model(mpm_ctx* ctx, int material, const mpm_material_params* params, const float* xyz, size_t n, const float v0[3], int* model_id) {
	return add_model(ctx, "mpm_add_model", material, params, xyz, n, v0, nullptr, model_id);
}

int mpm_add_model_particles(mpm_ctx* ctx, int material, const mpm_material_params* params, const float* xyz, size_t n, const float v0[3], const mpm_particle_init* init, int* model_id) {
	return add_model(ctx, init ? "mpm_add_model_particles" : "mpm_add_model", material, params, xyz, n, v0, init, model_id);
}

int mpm_set_model_velocity_field(mpm_ctx* ctx, int model, const float v0[3], const float grad9[9], const float pivot[3]) {
	if(!ctx) return MPM_ERR_INVALID;
	const std::string who = "mpm_set_model_velocity_field";
	if(ctx->ready) return fail(ctx, MPM_ERR_INVALID, who + ": the field is set before mpm_initial_setup");
	if(model < 0 || model >= (int) ctx->models.size()) return fail(ctx, MPM_ERR_INVALID, who + ": no model " + std::to_string(model));
	Model& m = ctx->models[model];
	if(m.d_init_velocity.n || m.d_init_affine.n) return fail(ctx, MPM_ERR_INVALID, who + ": the model was added with a velocity or affine9 array");
	VelocityField f {};
	for(int d = 0; d < 3; ++d) f.v0[d] = v0 ? v0[d] : 0.f, f.pivot[d] = pivot ? pivot[d] : 0.f;
	for(int d = 0; d < 9; ++d) f.G[d] = grad9 ? grad9[d] : 0.f;
	for(float x: f.v0)
		if(!std::isfinite(x)) return fail(ctx, MPM_ERR_INVALID, who + ": v0 is not finite");
	for(float x: f.G)
		if(!std::isfinite(x)) return fail(ctx, MPM_ERR_INVALID, who + ": grad9 is not finite");
	for(float x: f.pivot)
		if(!std::isfinite(x)) return fail(ctx, MPM_ERR_INVALID, who + ": pivot is not finite");
	m.field		= f;
	m.has_field = true;
	for(int d = 0; d < 3; ++d) m.v0[d] = f.v0[d];
	return MPM_OK;
}

// Host synchronisation with a short spin in front of the blocking wait: when the stream is about to drain (the end of a substep whose
// kernels are already running) the blocking wait's wake-up latency (~15-20 us) would sit between two substeps as GPU idle time.
static hipError_t sync_stream(hipStream_t s) {
	const auto t0 = std::chrono::steady_clock::now();
	for(;;) {
		const hipError_t q = hipStreamQuery(s);
		if(q != hipErrorNotReady) return q;
		if(std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(400)) break;
	}
	return hipStreamSynchronize(s);
}
static int read_status(mpm_ctx* ctx) {
	HIP_TRY(hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(int) * kStatusBlock, hipMemcpyDeviceToHost, ctx->s_compute));// status + halo counters + max |v|^2 slots
	HIP_TRY(sync_stream(ctx->s_compute));
	return MPM_OK;
}

static int check_status(mpm_ctx* ctx) {
	const int* st = ctx->h_status;
	if(st[ST_OVERFLOW] & 1) return fail(ctx, MPM_ERR_CAPACITY, "Too much active blocks: block capacity " + std::to_string(ctx->g.cap) + " exceeded");
	if((st[ST_OVERFLOW] & 2) && !ctx->cfg.drop_overflow) return fail(ctx, MPM_ERR_CAPACITY, "particles-per-block capacity exceeded (max_ppc*64 = " + std::to_string(ctx->g.ppb) + ")");
	if(st[ST_OVERFLOW] & 4) return fail(ctx, MPM_ERR_CAPACITY, "bin capacity exceeded");
	return MPM_OK;
}

// The particles one model is laid out from, in one order: set-up's own arrays, or the staging columns of an emission (mpm_particle_emit.hpp).
struct LayModel {
	size_t n;
	const float* xyz;
	ParticleInit init;
	bool with_state;// the bins take the material state from init (fill_bins_state_kernel), else the stress-free one (fill_bins_kernel)
	const int* staged_ids;// tracked contexts: the id of particle i (null: i itself, fill_ids_kernel)
};
// Model mi into the blocks of `table` (pbc particle blocks; the two partitions hold the same numbering): particles bucketed per block, bins handed out,
// bins and identity advection records filled, ids beside them.  m.list[1] is left holding the particle indices by block, m.size their counts.
static int lay_model_bins(mpm_ctx* ctx, size_t mi, const int* table, int pbc, const LayModel& in) {
	Model& m	  = ctx->models[mi];
	const GridCfg& g = ctx->g;
	hipStream_t s = ctx->s_compute;
	const int r = ctx->rollid, n = r ^ 1;
	HIP_TRY(hipMemsetAsync(m.keep, 0xff, sizeof(int) * ((size_t) g.cap + 1), s));
	if(in.n) bucket_particles_kernel<<<cdiv(in.n, 256), 256, 0, s>>>(g, in.n, in.xyz, table, m.out_count, m.list[1], ctx->d_status);
	if(pbc) {
		init_bins_kernel<<<cdiv(pbc, 256), 256, 0, s>>>(pbc, m.out_count, m.size, m.row_of, m.binoff[r], m.binoff[n], &ctx->d_status[ST_BINS0 + mi]);
		if(in.with_state)// a per-particle material state (mpm_particle_init.hpp)
			fill_bins_state_kernel<<<pbc, 256, 0, s>>>(g, m.nch, m.mc.log_jp0, in.xyz, m.list[1], m.size, m.binoff[r], m.bins[r], m.list[0], in.init);
		else
			fill_bins_kernel<<<pbc, 256, 0, s>>>(g, m.nch, m.mc.log_jp0, in.xyz, m.list[1], m.size, m.binoff[r], m.bins[r], m.list[0]);
		if(ctx->track_ids) {
			if(in.staged_ids)
				emit_fill_ids_kernel<<<pbc, 256, 0, s>>>(g.ppb, m.list[1], m.size, m.binoff[r], in.staged_ids, m.ids[r]);
			else
				fill_ids_kernel<<<pbc, 256, 0, s>>>(g.ppb, m.list[1], m.size, m.binoff[r], m.ids[r]);
		}
	}
	m.list_in = 0;
	return MPM_OK;
}

// initial_setup, gmpm_simulator.cuh:637-781
int mpm_initial_setup(mpm_ctx* ctx) {
	phase_call(ctx);
	if(!ctx || ctx->ready || ctx->models.empty()) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	GridCfg& g		   = ctx->g;
	hipStream_t s	   = ctx->s_compute;
	const size_t table = (size_t) g.G * g.G * g.G;
	const int r = ctx->rollid, n = r ^ 1;
	HIP_TRY(ctx->d_status.alloc(kStatusBlock, s));
	HIP_TRY(ctx->h_status.alloc(kStatusBlock));
	ctx->d_halo_counts = ctx->d_status + ST_WORDS;
	ctx->h_halo_counts = ctx->h_status + ST_WORDS;
	ctx->d_peer_rows   = ctx->d_halo_counts + 2 + 32;
	ctx->h_peer_rows   = ctx->h_halo_counts + 2 + 32;
	ctx->d_maxvel	   = reinterpret_cast<unsigned*>(ctx->d_status + ST_WORDS + kHaloWords);
	ctx->h_maxvel	   = reinterpret_cast<float*>(ctx->h_status + ST_WORDS + kHaloWords);
	ctx->d_stamps	   = reinterpret_cast<unsigned long long*>(ctx->d_status + kStatusCore);
	ctx->h_stamps	   = reinterpret_cast<const unsigned long long*>(ctx->h_status + kStatusCore);
	HIP_TRY(ctx->d_totals.alloc(4, s));
	HIP_TRY(ctx->d_counter.alloc(1, s));
	for(int i = 0; i < 2; ++i) {
		HIP_TRY(ctx->part[i].table.alloc(table, s));
		HIP_TRY(ctx->part[i].count.alloc(1, s));
		HIP_TRY(hipMemsetAsync(ctx->part[i].table, 0xff, sizeof(int) * table, s));
	}
	// Pass 1: activate particle blocks with a provisional capacity = table size bound by the particle count
	size_t total_particles = 0;
	for(auto& m: ctx->models) total_particles += m.n;
	size_t prov = std::min(table, total_particles + 1);
	if(ctx->cfg.max_blocks > 0) prov = std::min<size_t>(table, (size_t) ctx->cfg.max_blocks);
	Partition& P = ctx->part[n];
	HIP_TRY(P.keys.alloc(3 * prov, s));
	g.cap = (int) prov;
	for(auto& m: ctx->models)
		if(m.n) activate_blocks_kernel<<<cdiv(m.n, 256), 256, 0, s>>>(g, m.n, m.d_xyz, P.table, P.keys, P.count, ctx->d_status);
	int pbc = 0;
	HIP_TRY(hipMemcpyAsync(&pbc, P.count, sizeof(int), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if(pbc > g.cap) return fail(ctx, MPM_ERR_CAPACITY, "Too much active blocks: " + std::to_string(pbc));
	ctx->pbc = pbc;
	// neighbours, exterior (gmpm_simulator.cuh:706-734) - registered now, still in the provisional key list, so that the
	// capacities below can be sized by the exterior block count that is actually there (a compact body has ~1.15 exterior
	// blocks per particle block, a thin sheet up to 27: sizing by a fixed multiple of pbc wasted 8 GB at C3)
	if(ctx->cfg.max_blocks <= 0 && (size_t) pbc * 27 > prov) {// the provisional list must hold every block that can be registered
		prov = std::min(table, (size_t) pbc * 27 + 1);
		HIP_TRY(P.keys.grow(3 * prov, s));
		g.cap = (int) prov;
	}
	// (one-time set-up: the phase counters start from the activation's count; the published counts are formed on the host below)
	HIP_TRY(hipMemcpyAsync(&ctx->d_status[ST_CNT_P], P.count, sizeof(int), hipMemcpyDeviceToDevice, s));
	register_blocks_kernel<0, 1><<<std::max(1u, std::min(4096u, cdiv((size_t) pbc * 8, 256))), 256, 0, s>>>(g, &ctx->d_status[ST_CNT_P], nullptr, &ctx->d_status[ST_CNT_N], &ctx->d_status[ST_PBC], P.table, P.keys, ctx->d_status, 0);
	register_blocks_kernel<-1, 1><<<std::max(1u, std::min(8192u, cdiv((size_t) pbc * 32, 256))), 256, 0, s>>>(g, &ctx->d_status[ST_CNT_P], &ctx->d_status[ST_CNT_N], &ctx->d_status[ST_CNT_E], &ctx->d_status[ST_NBC], P.table, P.keys, ctx->d_status, 0);
	{
		int rc0 = read_status(ctx);
		if(rc0) return rc0;
		rc0 = check_status(ctx);
		if(rc0) return rc0;
		const int ebc0 = ctx->h_status[ST_CNT_P] + ctx->h_status[ST_CNT_N] + ctx->h_status[ST_CNT_E];
		ctx->h_status[ST_EBC] = ebc0;
		ctx->pbc_prev		  = pbc;
		HIP_TRY(hipMemcpyAsync(&ctx->d_status[ST_EBC], &ctx->h_status[ST_EBC], sizeof(int), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(&ctx->d_status[ST_PBCPREV], &ctx->pbc_prev, sizeof(int), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(P.count, &ctx->h_status[ST_EBC], sizeof(int), hipMemcpyHostToDevice, s));
		HIP_TRY(hipStreamSynchronize(s));
	}
	ctx->nbc = ctx->h_status[ST_NBC];
	ctx->ebc = ctx->h_status[ST_EBC];
	// final capacity (reference: compile-time G_MAX_ACTIVE_BLOCK, grown by 1.5x on demand, gmpm_simulator.cuh:283-300):
	// 3/2 of the exterior blocks + slack, i.e. below the 3/4 fill level at which check_capacity() grows it
	size_t cap = ctx->cfg.max_blocks > 0 ? (size_t) ctx->cfg.max_blocks : std::min(table, (size_t) ctx->ebc * 3 / 2 + 4096);
	if(cap < (size_t) ctx->ebc) return fail(ctx, MPM_ERR_CAPACITY, "Too much exterior blocks: " + std::to_string(ctx->ebc) + " (max_blocks " + std::to_string(cap) + ")");
	if(P.keys.n > 3 * cap) {// the provisional list was the longer one: the final one holds the registered keys alone
		DevBuf<int> keys;
		HIP_TRY(keys.alloc(3 * cap, s));
		HIP_TRY(hipMemcpyAsync(keys, P.keys, sizeof(int) * 3 * (size_t) ctx->ebc, hipMemcpyDeviceToDevice, s));
		HIP_TRY(hipStreamSynchronize(s));
		P.keys = std::move(keys);
	}
	g.cap = (int) cap;
	for(auto& m: ctx->models) m.pair = ((pair_mask() >> m.material) & 1) != 0 && g.ppb <= kPairChunks * kListChunk;
	HIP_TRY(size_block_arrays(ctx, cap, false));
	// per model: bucket particles per block, allocate bins, fill bins + identity advection records
	for(size_t mi = 0; mi < ctx->models.size(); ++mi) {
		Model& m  = ctx->models[mi];
		m.bin_cap = m.n / kBin + cap + 1;
		HIP_TRY(size_bin_arrays(ctx, m, m.bin_cap));
		if(int rc = lay_model_bins(ctx, mi, P.table, pbc, {m.n, m.d_xyz, particle_init_view(m), m.d_init_state.n || m.d_init_logjp.n, nullptr})) return rc;
	}
	int rc = read_status(ctx);// bin totals of the models
	if(rc) return rc;
	rc = check_status(ctx);
	if(rc) return rc;
	// a block that STARTS with more particles than it has list slots is a configuration error whatever the overflow policy (the drop
	// policy covers particles that arrive at run time: a dropped particle must not have been rasterised)
	if(ctx->h_status[ST_OVERFLOW] & 2) return fail(ctx, MPM_ERR_CAPACITY, "a block holds more than max_ppc*64 = " + std::to_string(g.ppb) + " particles at set-up");
	if(ctx->h_status[ST_LOST]) return fail(ctx, MPM_ERR_INVALID, "particles outside the domain at setup");
	for(size_t mi = 0; mi < ctx->models.size(); ++mi) {
		ctx->models[mi].bincount = ctx->h_status[ST_BINS0 + mi];
		ctx->models[mi].bincount_src = ctx->models[mi].bincount;
		ctx->models[mi].bucketed = (int64_t) ctx->models[mi].n;
		if((size_t) ctx->models[mi].bincount > ctx->models[mi].bin_cap) return fail(ctx, MPM_ERR_CAPACITY, "bin capacity");
	}
	// copy the partition to the other roll (gmpm_simulator.cuh:745-748): previous numbering == current numbering
	HIP_TRY(hipMemcpyAsync(ctx->part[r].table, P.table, sizeof(int) * table, hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipMemcpyAsync(ctx->part[r].keys, P.keys, sizeof(int) * 3 * (size_t) ctx->ebc, hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipMemcpyAsync(ctx->part[r].count, P.count, sizeof(int), hipMemcpyDeviceToDevice, s));
	// rasterize (gmpm_simulator.cuh:763-771)
	HIP_TRY(hipMemsetAsync(ctx->grid[0], 0, sizeof(float) * 256 * (size_t) ctx->nbc, s));
	for(auto& m: ctx->models) {// (m.list[1] still holds the particle ids by block that bucket_particles_kernel wrote; every particle of the model is in a block: ST_LOST was checked above)
		if(!m.n || !pbc) continue;
		VelocityField f = m.field;
		for(int d = 0; d < 3; ++d) f.v0[d] = m.v0[d];
		if(m.has_field)// per-particle velocities (mpm_particle_init.hpp): from a field, or from the model's arrays
			rasterize_particles_kernel<true><<<pbc, 256, 0, s>>>(g, m.d_xyz, m.list[1], m.size, ctx->part[r].keys, ctx->part[r].table, ctx->grid[0], m.mc.mass, ParticleInit {}, f);
		else if(m.d_init_velocity.n || m.d_init_affine.n)
			rasterize_particles_kernel<false><<<pbc, 256, 0, s>>>(g, m.d_xyz, m.list[1], m.size, ctx->part[r].keys, ctx->part[r].table, ctx->grid[0], m.mc.mass, particle_init_view(m), f);
		else
			rasterize_blocks_kernel<<<pbc, 256, 0, s>>>(g, m.d_xyz, m.list[1], m.size, ctx->part[r].keys, ctx->part[r].table, ctx->grid[0], m.mc.mass, m.v0[0], m.v0[1], m.v0[2]);
	}
	// the first G2P2G: current == previous numbering (roll r), lists as filled above
	rc = launch_prepare(ctx, PrepareFor::Setup);
	if(rc) return rc;
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	for(auto& m: ctx->models)// the per-particle initial conditions have been used
		for(DevBuf<float>* b: {&m.d_init_velocity, &m.d_init_affine, &m.d_init_state, &m.d_init_logjp}) (void) b->reset();
	ctx->ready		   = true;
	ctx->relaid		   = true;
	ctx->grid_momentum = true;
	ctx->ids_valid	   = ctx->track_ids;
	return MPM_OK;
}

// The pivots of the load rows: the collider's shift at T (collision_pose's own statement) unless the caller gave one; the walls' default is the origin.
static LoadPivots load_pivots(const mpm_ctx* ctx, const mpm_load_options* opt) {
	LoadPivots piv {};
	const float T = ctx->collision.time;
	for(int r = 0; r < kLoadRows; ++r) {
		const CollisionObject* o = nullptr;// the row's collider, if one is installed
		if(r == 0 && ctx->has_collision) o = &ctx->collision;
		if(r >= 1 && r <= kMaxShapes && r - 1 < ctx->shape_count && ctx->shape[r - 1].shape.kind) o = &ctx->shape[r - 1].obj;
		for(int d = 0; d < 3; ++d) {
			if(opt && opt->has_pivot[r])
				piv.p[r][d] = (double) opt->pivot[r][d];
			else if(o)
				piv.p[r][d] = (double) (r >= 1 && ctx->frozen[r - 1] ? ctx->frozen_pose[r - 1] : collision_pose(*o, T)).shift[d];
		}
	}
	return piv;
}
// collider_loads_kernel and its reduction on the compute stream: the totals of the update that dt would apply now into out (accumulate 0) or
// added to out, with dt and the call count behind them (accumulate 1).  partials: kLoadGroups x [kLoadRows][kLoadSums] doubles.
// forces: the fields the coming update's pre-pass will apply (the readout), or none when that pass has run already (the gauge).
static int launch_collider_loads(mpm_ctx* ctx, float dt, const mpm_load_options* opt, double* partials, double* out, int accumulate, const ForceArgs& forces) {
	hipStream_t s		 = ctx->s_compute;
	const LoadPivots piv = load_pivots(ctx, opt);
	int state_pivots	 = ctx->body_mask;// a body row's default pivot is its x, read on the device
	for(int i = 0; i < kMaxBodies; ++i)
		if(opt && opt->has_pivot[1 + i]) state_pivots &= ~(1 << i);
	with_collider_at_clock(ctx, [&](const auto& col) { collider_loads_kernel<<<kLoadGroups, 256, 0, s>>>(ctx->g, &ctx->d_status[ST_NBC], ctx->grid[0], ctx->part[ctx->rollid].keys, dt, col, piv, partials, forces); }, state_pivots);
	collider_loads_reduce_kernel<<<1, kLoadReduceThreads, 0, s>>>(partials, kLoadGroups, out, accumulate, (double) dt);
	HIP_TRY(hipGetLastError());
	return MPM_OK;
}

// grid-update phase, gmpm_simulator.cuh:326-347
static int launch_grid_update(mpm_ctx* ctx, float dt) {
	hipStream_t s = ctx->s_compute;
	// the force fields' pass over the momenta (mpm_force_field.hpp), ahead of everything that reads them: the gauge, the bodies, the update
	if(ctx->force.count > 0 && !ctx->grid_preupdated && ctx->nbc) {
		const int est = std::min(ctx->g.cap, ctx->nbc + ctx->nbc / 16 + 64);
		grid_force_kernel<<<cdiv(est, 4), 256, 0, s>>>(ctx->g, &ctx->d_status[ST_NBC], ctx->grid[0], ctx->part[ctx->rollid].keys, dt, ctx->force);
	}
	// the load gauge reads the momenta this update is about to turn into velocities (a grid that holds none, or a grouped context's, is not read)
	if(ctx->load_gauge && ctx->grid_momentum && !ctx->grid_preupdated && ctx->group_refs == 0 && ctx->mgsp_rank < 0 && !ctx->halo_tagged)
		if(int rc = launch_collider_loads(ctx, dt, &ctx->load_opt, ctx->d_load_partials, ctx->d_load_acc, 1, ForceArgs {})) return rc;
	ctx->grid_momentum = false;// (from here on grid[0] holds velocities, until a rebuild carries the next P2G over)
	if(ctx->grid_preupdated) {
		ctx->grid_preupdated = false;
		if(dt != ctx->preupdate_dt) return fail(ctx, MPM_ERR_INVALID, "grid was updated for another dt");
		return MPM_OK;// (the carry-over that applied this update has advanced the object's clock)
	}
	HIP_TRY(hipMemsetAsync(ctx->d_maxvel, 0, sizeof(unsigned) * kMaxVelSlots * kMaxVelStride, s));
	if(!ctx->nbc && !ctx->body_mask) return MPM_OK;// (no block: no update is applied)
	const int est = std::min(ctx->g.cap, ctx->nbc + ctx->nbc / 16 + 64);// (an estimate between two synchronisations of mpm_run_fixed)
	const LoadPivots piv = ctx->body_mask ? load_pivots(ctx, nullptr) : LoadPivots {};// (at the clock's time before this update moves it)
	with_collider(ctx, dt, [&](const auto& col) {
		using Collider = std::decay_t<decltype(col)>;
		if constexpr(kCarriesBodies<Collider>) {// the update and its loads in one pass, then the bodies' step (mpm_rigid_body.hpp); the clock moves as for any applied update
			grid_update_body_kernel<<<kLoadGroups, 256, 0, s>>>(ctx->g, &ctx->d_status[ST_NBC], ctx->grid[0], ctx->part[ctx->rollid].keys, dt, col, piv, ctx->d_body_partials, ctx->d_maxvel);
			body_step_kernel<<<1, kLoadReduceThreads, 0, s>>>(ctx->d_body_partials, kLoadGroups, ctx->d_body, ctx->body_mask, dt, ctx->cfg.gravity, &ctx->d_status[ST_NONFINITE]);
		} else if constexpr(!kCollides<Collider>)
			grid_update_kernel<<<cdiv(est, 16), 256, 0, s>>>(ctx->g, &ctx->d_status[ST_NBC], ctx->grid[0], ctx->part[ctx->rollid].keys, dt, ctx->d_maxvel);
		else
			grid_update_collider_kernel<<<cdiv(est, 4), 256, 0, s>>>(ctx->g, &ctx->d_status[ST_NBC], ctx->grid[0], ctx->part[ctx->rollid].keys, dt, col, ctx->d_maxvel);
	}, ctx->body_mask);
	if(ctx->body_mask) HIP_TRY(hipGetLastError());
	return MPM_OK;
}

int mpm_grid_update(mpm_ctx* ctx, float dt, float* max_vel_sqr) {
	phase_call(ctx);
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	HIP_TRY(hipEventRecord(ctx->ev.start, s));
	int rc = launch_grid_update(ctx, dt);
	if(rc) return rc;
	HIP_TRY(hipEventRecord(ctx->ev.end, s));
	HIP_TRY(hipMemcpyAsync(ctx->h_maxvel, ctx->d_maxvel, sizeof(float) * kMaxVelSlots * kMaxVelStride, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	HIP_TRY(hipEventElapsedTime(&ctx->timers.grid_update_ms, ctx->ev.start, ctx->ev.end));
	if(max_vel_sqr) *max_vel_sqr = host_maxvel(ctx);
	return MPM_OK;
}

float mpm_compute_dt(const mpm_ctx* ctx, float max_vel, float cur_time, float next_time, float dt_default) {
	// utility_funcs.hpp:36-49
	float dt = dt_default;
	if(max_vel > 0.0f) dt = std::min(ctx->g.dx * ctx->cfg.cfl / max_vel, dt);
	return std::min(dt, next_time - cur_time);
}

static ModelView make_view(mpm_ctx* ctx, Model& m) {
	const int r = ctx->rollid, n = r ^ 1;
	ModelView v {};
	v.bins_src	 = m.bins[r];
	v.bins_dst	 = m.bins[n];
	v.binoff_src = m.binoff[r];
	v.binoff_dst = m.binoff[n];
	v.list_in	 = m.list[m.list_in];
	v.list_out	 = m.list[m.list_in ^ 1];
	v.size		 = m.size;
	v.row_of	 = m.row_of;
	v.out_count	 = m.out_count;
	v.keep		 = m.keep;
	v.blockinfo	 = m.blockinfo;
	v.pairinfo_in  = m.pairinfo[0];
	v.pairinfo_out = m.pairinfo[1];
	v.mc		 = m.mc;
	return v;
}

// Model m as every readout reads it (mpm_readout.hpp): its list and bins, in the numberings of the last rebuild.
static ReadoutArgs make_readout_args(mpm_ctx* ctx, const Model& m) {
	const int r = ctx->rollid;
	return ReadoutArgs {ctx->g, m.nch, m.pair ? 1 : 0, ctx->part[r].keys, ctx->part[r].table, ctx->part[r ^ 1].table, m.size, m.row_of, m.list[m.list_in], m.binoff[r], m.bins[r], m.ids[r]};
}

// a launch size for `n` (an estimate that may be a few substeps old) particle blocks: margin for growth, a multiple of 8 (XCDs)
static inline int hint_blocks(const mpm_ctx* ctx, int n) {
	const long long h = (long long) n + n / 16 + 64;
	return (int) ((std::min<long long>(h, std::max(ctx->g.cap, 8)) + 7) & ~7ll);
}

// nblocks_ptr != nullptr: the block count is read from device memory, `nblocks` is the host's estimate of it (launch size);
// otherwise `nblocks` is exact (the halo / interior lists of the MGSP path, whose lengths the host has read back)
static void launch_g2p2g_model(mpm_ctx* ctx, const SubstepPlan& plan, Model& m, const int* block_list, const int* nblocks_ptr, int nblocks, hipStream_t s, const int* only_flag = nullptr) {
	const int r = ctx->rollid;
	const float dt = plan.dt, next_dt = plan.next_dt;
	ModelView v = make_view(ctx, m);
	const int* cur_keys	  = ctx->part[r].keys;
	const GridCfg& g = ctx->g;
	StepConst sk;
	sk.dtp	= dt * g.dx_inv;
	sk.dts	= dt * (4.f * g.dx_inv);
	sk.pred = next_dt * g.dx_inv;
	sk.am	= m.mc.mass * g.dx * g.dx * g.d_inv;
	const float cs = -next_dt * g.d_inv * g.dx;// the stress enters the P2G payload as -P F^T vol new_dt D^-1 dx (:850)
	sk.ss	= StressScale {2.f * m.mc.mu * m.mc.volume * cs, m.mc.lambda * m.mc.volume * cs, m.mc.volume * cs};
	sk.refl_lim = sk.dts > 0.f ? (1.f / 3.f) / sk.dts : 3.0e38f;
	sk.jdiv		= g.dx * dt * g.d_inv;
	sk.jvisc	= g.dx * g.d_inv * m.mc.viscosity;
	sk.stamp	= plan.stamp_row && &m == &ctx->models.front() ? plan.stamp_row + 1 : nullptr;
	const int nwg = nblocks_ptr ? hint_blocks(ctx, nblocks) : nblocks;
	auto kernel = g2p2g_for<3>(m.pair);
	switch(m.material) {
		case MPM_J_FLUID: kernel = g2p2g_for<0>(m.pair); break;
		case MPM_FIXED_COROTATED: kernel = g2p2g_for<1>(m.pair); break;
		case MPM_SAND: kernel = g2p2g_for<2>(m.pair); break;
		default: break;
	}
	kernel<<<nwg, kG2P2GThreads, 0, s>>>(ctx->g, v, cur_keys, ctx->grid[0], ctx->grid[1], block_list, only_flag, nblocks_ptr, nblocks, dt, next_dt, sk, ctx->d_status);
	// tracked context: the identities take the same step, from what this launch has just been given (mpm_particle_ids.hpp)
	if(ctx->track_ids && nwg > 0) {
		const MoveIdsArgs a {g.ppb, g.pid_bits, g.cap, m.pair ? 1 : 0, v.size, v.row_of, v.list_in, v.binoff_dst, v.blockinfo, m.ids[r], m.ids[r ^ 1]};
		move_ids_kernel<<<cdiv((size_t) nwg, kMoveIdsWaves), kMoveIdsThreads, 0, s>>>(a, block_list, only_flag, nblocks_ptr, nblocks);
	}
}

// substep_clear_kernel: the P2G part precedes G2P2G (clear_grid + the bucket counters, gmpm_simulator.cuh:383,:389), the rebuild
// part precedes the rebuild (reset_table + the counters, :436-446); plan.rebuild_clear issues both in one launch
static int launch_clear(mpm_ctx* ctx, const SubstepPlan& plan, int flags) {
	if((flags & kClearRebuild) && !(flags & kClearP2G)) {// called by the rebuild itself
		if(ctx->rebuild_cleared) flags &= ~(kClearRebuild | kClearMaxVel);// (already issued with this substep's P2G part)
		ctx->rebuild_cleared = false;
	}
	if(!(flags & (kClearP2G | kClearRebuild))) return MPM_OK;
	ClearArgs a {};
	a.flags	  = flags;
	a.nmodels = (int) ctx->models.size();
	for(int mi = 0; mi < a.nmodels; ++mi) a.out_count[mi] = ctx->models[mi].out_count, a.keep[mi] = ctx->models[mi].keep;
	a.p2g_grid	   = ctx->grid[1];
	a.status	   = ctx->d_status;
	a.max_vel_bits = ctx->d_maxvel;
	Partition& Pn  = ctx->part[ctx->rollid ^ 1];
	a.old_table	   = Pn.table;
	a.old_keys	   = Pn.keys;
	a.old_count	   = Pn.count;
	a.stamp		   = (flags & kClearP2G) ? plan.stamp_row : nullptr;// (the substep's first launch)
	substep_clear_kernel<<<1024, 256, 0, ctx->s_compute>>>(ctx->g, a);
	return MPM_OK;
}
// (with plan.fuse_dt the rebuild's carry-over applies the next grid update, i.e. writes the max |v|^2 slots: the clear that rides along resets them)
static int launch_g2p2g_prologue(mpm_ctx* ctx, const SubstepPlan& plan) {
	int rc = launch_clear(ctx, plan, plan.rebuild_clear ? (kClearP2G | kClearRebuild | (plan.fuse_dt > 0.f ? kClearMaxVel : 0)) : kClearP2G);
	if(rc == MPM_OK && plan.rebuild_clear) ctx->rebuild_cleared = true;
	return rc;
}

static int launch_g2p2g(mpm_ctx* ctx, const SubstepPlan& plan) {
	hipStream_t s = ctx->s_compute;
	int rc		  = launch_g2p2g_prologue(ctx, plan);
	if(rc) return rc;
	if(plan.ev.g2p2g_start) HIP_TRY(hipEventRecord(plan.ev.g2p2g_start, s));// (null events: a substep of mpm_run_fixed whose kernels stamp their phases)
	if(ctx->pbc)
		for(auto& m: ctx->models) launch_g2p2g_model(ctx, plan, m, nullptr, &ctx->d_status[ST_PBC], ctx->pbc, s);
	if(plan.ev.g2p2g_end) HIP_TRY(hipEventRecord(plan.ev.g2p2g_end, s));
	return MPM_OK;
}

int mpm_g2p2g(mpm_ctx* ctx, float dt, float next_dt) {
	phase_call(ctx);
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	int rc = launch_g2p2g(ctx, default_plan(ctx, dt, next_dt));
	if(rc) return rc;
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(ctx->s_compute));
	HIP_TRY(hipEventElapsedTime(&ctx->last_g2p2g_ms, ctx->ev.g2p2g_start, ctx->ev.g2p2g_end));
	ctx->timers.g2p2g_ms = ctx->last_g2p2g_ms;
	return MPM_OK;
}

// Per-block preparation of the next G2P2G (prepare_blocks_kernel).  Set-up and a checkpoint load prepare the current numbering r, in which the
// particle data is laid out too, from the lists G2P2G reads next (set-up sorts them, a checkpoint's are sorted).  The rebuild's last kernel prepares
// the new numbering n with the data laid out in r: it sorts the lists the last G2P2G appended to (the only call that hands on `keep`), publishes the
// exterior block count, may take the still path and follows the still streak (thin: what launch_rebuild resolved).  The launch is sized by the host's
// estimate of the block count the kernel reads from the status block; the kernel walks over what is beyond it.
static int launch_prepare(mpm_ctx* ctx, PrepareFor why, const StillLaunch& thin) {
	const bool rebuild = why == PrepareFor::Rebuild;
	const int r = ctx->rollid, cur = rebuild ? r ^ 1 : r, prev = cur ^ 1;
	const int nblocks_est = rebuild ? std::min(ctx->g.cap, ctx->ebc + ctx->ebc / 16 + 1024) : ctx->pbc;
	if(nblocks_est <= 0 && !rebuild) return MPM_OK;
	PrepareModels pm {};
	pm.n = (int) ctx->models.size();
	for(int mi = 0; mi < pm.n; ++mi) {
		Model& m		  = ctx->models[mi];
		pm.list[mi]		  = m.list[rebuild ? (m.list_in ^ 1) : m.list_in];
		pm.size[mi]		  = m.size;
		pm.row_of[mi]	  = m.row_of;
		pm.binoff_src[mi] = m.binoff[cur];
		pm.blockinfo[mi]  = m.blockinfo;
		pm.keep[mi]		  = rebuild ? m.keep : nullptr;
		pm.pairinfo[mi]	  = m.pair ? m.pairinfo[0] : nullptr;
		pm.pairhand[mi]	  = m.pairinfo[1];
	}
	int nwg = std::max(1, std::min(ctx->g.cap, nblocks_est + nblocks_est / 16 + 64));
	if(rebuild && thin.prepare > 0) nwg = std::min(nwg, thin.prepare);// (still_launch_rule)
	const int* pbc_ptr = &ctx->d_status[rebuild ? ST_CNT_P : ST_PBC];
	int* pub		   = rebuild ? ctx->d_status : nullptr;// (... and publishes the exterior block count)
	auto kernel		   = why != PrepareFor::CheckpointLoad ? prepare_blocks_kernel<true> : prepare_blocks_kernel<false>;// (a checkpoint's lists are sorted)
	kernel<<<nwg, 64, 0, ctx->s_compute>>>(ctx->g, pm, pbc_ptr, ctx->part[cur].table, ctx->part[cur].keys, ctx->part[prev].table, pub, ctx->part[cur].count, rebuild ? thin.still : 0);
	return MPM_OK;
}

// partition rebuild, gmpm_simulator.cuh:415-579 (launches only: no host round trip, no runtime fill / copy commands; launch sizes
// from the host's estimates of the block counts, true counts from the status block)
// (plan.fuse_dt, plan.offer_still: SubstepPlan; the still path is not taken when the data was laid out anew since the last rebuild)
// tail != null: everything but the last kernel (prepare_blocks_kernel: list sort, look-up rows, publication of the exterior block count), which
// launch_rebuild_prepare issues with *tail - the group loop puts the tagging's key export in between, so that the key all-gather and the tagging
// kernels run on the comm stream beside it
static int launch_rebuild_prepare(mpm_ctx* ctx, const StillLaunch& thin) {
	return launch_prepare(ctx, PrepareFor::Rebuild, thin);
}
static int launch_rebuild(mpm_ctx* ctx, const SubstepPlan& plan, StillLaunch* tail) {
	const float fuse_dt = plan.fuse_dt;
	hipStream_t s = ctx->s_compute;
	GridCfg& g	  = ctx->g;
	const int r = ctx->rollid, n = r ^ 1;
	Partition& Pn = ctx->part[n];
	Partition& Pr = ctx->part[r];
	const bool fused = fuse_dt > 0.f;
	if(fused && ctx->body_mask) return fail(ctx, MPM_ERR_INTERNAL, "a grid update with a rigid body installed cannot ride on the carry-over (it has no BodyArgs instantiation)");
	if(fused && ctx->force.count) return fail(ctx, MPM_ERR_INTERNAL, "a grid update with a force field installed cannot ride on the carry-over (the fields' pass runs ahead of a stand-alone update)");
	const int still = plan.offer_still && !ctx->relaid ? 1 : 0;
	ctx->relaid		= false;
	ctx->grid_momentum = !fused;// the carry-over below writes grid[0]: the P2G's mass and momentum, or (fused) the updated velocities
	int rc			 = launch_clear(ctx, plan, kClearRebuild | (fused ? kClearMaxVel : 0));// un-insert the old keys of Pn (reset_table, hash_table.cuh:110-112), counters, totals
	if(rc) return rc;
	RebuildModels rm {};
	rm.n = (int) ctx->models.size();
	for(int mi = 0; mi < rm.n; ++mi) {
		Model& m		 = ctx->models[mi];
		rm.out_count[mi] = m.out_count;
		rm.size[mi]		 = m.size;
		rm.row_of[mi]	 = m.row_of;
		rm.binoff[mi]	 = m.binoff[r];// becomes the destination offsets after the roll
		rm.binoff_cur[mi] = m.binoff[n];
		rm.bin_cap[mi]	 = (long long) m.bin_cap;
	}
	int* st			  = ctx->d_status;
	const int ebc_est = std::min(g.cap, ctx->ebc + ctx->ebc / 16 + 1024);
	compact_blocks_kernel<<<std::max(1u, cdiv(ebc_est, 1024)), 1024, 0, s>>>(g, rm, Pr.keys, Pn.keys, Pn.table, st, still, plan.stamp_row ? plan.stamp_row + 2 : nullptr);
	// (a rebuild that is not offered the still path - the host laid the data out anew, or another driver's - ends the streak whatever the last read-back said)
	if(!still) ctx->streak_seen = 0;
	StillLaunch thin = still_launch_rule(ctx->streak_seen, still != 0, ctx->pbc, ctx->still_launch);
	thin.still		 = still;
	unsigned rg8 = std::max(1u, std::min(4096u, cdiv((size_t) ebc_est * 8, 256))), rg32 = std::max(1u, std::min(8192u, cdiv((size_t) ebc_est * 32, 256)));
	if(thin.reg > 0) rg8 = std::min(rg8, (unsigned) thin.reg), rg32 = std::min(rg32, (unsigned) thin.reg);
	register_blocks_kernel<0, 1><<<rg8, 256, 0, s>>>(g, &st[ST_CNT_P], nullptr, &st[ST_CNT_N], &st[ST_PBC], Pn.table, Pn.keys, st, still);
	if(fused) {
		with_collider(ctx, fuse_dt, [&](const auto& col) {
			if constexpr(!kCarriesBodies<std::decay_t<decltype(col)>>)// (no driver fuses an update with a body installed: refused above)
				carry_grid_kernel<true, std::decay_t<decltype(col)>><<<2048, 256, 0, s>>>(g, st, Pn.keys, Pr.table, ctx->grid[1], ctx->grid[0], fuse_dt, ctx->d_maxvel, col);
		});
		ctx->grid_preupdated = true;
		ctx->preupdate_dt	 = fuse_dt;
	} else
		carry_grid_kernel<false><<<2048, 256, 0, s>>>(g, st, Pn.keys, Pr.table, ctx->grid[1], ctx->grid[0], 0.f, nullptr, NoCollision {});
	register_blocks_kernel<-1, 1><<<rg32, 256, 0, s>>>(g, &st[ST_CNT_P], &st[ST_CNT_N], &st[ST_CNT_E], &st[ST_NBC], Pn.table, Pn.keys, st, still);
	// the next G2P2G runs in the new numbering n with the particle data laid out in r: sort its lists (the ones the last
	// G2P2G appended to), look up its blocks' neighbours; this last kernel also publishes the exterior block count
	if(tail) return *tail = thin, MPM_OK;
	return launch_prepare(ctx, PrepareFor::Rebuild, thin);
}

// check_capacity() (gmpm_simulator.cuh:283-300): once the exterior block count / a model's bin count passes 3/4 of its
// capacity the capacity grows by 3/2.  Runs at a host synchronisation, after a rebuild; every
// array indexed by block number (keys, grids, lists, sizes, bin offsets, halo lists) or by bin is reallocated and
// copied.  The dense table is sized by the domain, not by the capacity.
// The two MECHANISMS: both streams idle (buffers are about to be replaced), every array of the roster grown, then the books.
static int reserve_blocks(mpm_ctx* ctx, size_t ncap) {
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(size_block_arrays(ctx, ncap, true));
	ctx->g.cap	= (int) ncap;
	ctx->relaid = true;
	ctx->capacity_events++;
	return MPM_OK;
}
static int reserve_bins(mpm_ctx* ctx, Model& m, size_t nb) {
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(size_bin_arrays(ctx, m, nb));
	m.bin_cap	= nb;
	ctx->relaid = true;
	ctx->capacity_events++;
	return MPM_OK;
}
// The POLICY.  Bins: past 3/4 full by 3/2, and never below the worst case of the block capacity - every block ends with one partially filled bin.
static int grow_bins(mpm_ctx* ctx) {
	for(auto& m: ctx->models) {
		const size_t need = m.n / kBin + (size_t) ctx->g.cap + 1;
		if((size_t) m.bincount * 4 > m.bin_cap * 3 || need > m.bin_cap)
			if(int rc = reserve_bins(ctx, m, std::max(need, (size_t) m.bincount * 4 > m.bin_cap * 3 ? m.bin_cap * 3 / 2 + 1 : m.bin_cap))) return rc;
	}
	return MPM_OK;
}
static int grow_capacity(mpm_ctx* ctx) {
	if(!ctx->cfg.grow) return MPM_OK;
	const size_t table = (size_t) ctx->g.G * ctx->g.G * ctx->g.G;
	const size_t cap   = (size_t) ctx->g.cap;
	if((size_t) ctx->ebc * 4 > cap * 3 && cap < table)
		if(int rc = reserve_blocks(ctx, std::min(table, cap * 3 / 2 + 1))) return rc;
	return grow_bins(ctx);
}

// the host's half of a rebuild that needs no device data: the roll (gmpm_simulator.cuh:578)
static void roll_partition(mpm_ctx* ctx) {
	for(auto& m: ctx->models) m.list_in ^= 1;
	ctx->rollid ^= 1;
}

// The library checks its own books at every host synchronisation (the reference prints the particle total per frame and leaves the
// reading to the user, gmpm_simulator.cuh:617): every particle that was added is either bucketed in a block of the partition just
// built, or was counted as lost (left the domain / a block nobody registered, particle_buffer.cuh:105-113) or as dropped (overflow
// policy).  The lost / dropped counters are per context, so the per-model statement is made when both are zero - the normal case -
// and the totals are compared otherwise.  A failure is a bug of the engine (round 4's windowed group loop skipped a launch and lost
// the particles of a few blocks with nothing counted as lost), never of the caller: MPM_ERR_INTERNAL.
static int check_books(mpm_ctx* ctx) {
	// (books_bias: what a loaded checkpoint's state was missing beyond this context's own counters - zero otherwise)
	const long long gone = (long long) ctx->h_status[ST_LOST] + (long long) ctx->h_status[ST_DROPPED] + ctx->books_bias;
	long long added = 0, held = 0;
	for(size_t mi = 0; mi < ctx->models.size(); ++mi) {
		const Model& m = ctx->models[mi];
		added += (long long) m.n;
		held += (long long) m.bucketed;
		if(gone == 0 && (long long) m.bucketed != (long long) m.n)
			return fail(ctx, MPM_ERR_INTERNAL,
						"particle books of model " + std::to_string(mi) + " do not balance: " + std::to_string(m.bucketed) + " bucketed of " + std::to_string(m.n) +
							" added, none counted as lost or dropped");
	}
	if(held + gone != added)
		return fail(ctx, MPM_ERR_INTERNAL,
					"particle books do not balance: " + std::to_string(held) + " bucketed + " + std::to_string(ctx->h_status[ST_LOST]) + " lost + " + std::to_string(ctx->h_status[ST_DROPPED]) +
						" dropped != " + std::to_string(added) + " added");
	return MPM_OK;
}

// Host synchronisation after one or more enqueued substeps (every one already rolled on the host): read the status block,
// report what went wrong in the meantime (flags are sticky), take over the counts, grow capacities.
static int apply_status(mpm_ctx* ctx, mpm_counts* counts);
static int sync_counts(mpm_ctx* ctx, mpm_counts* counts) {
	int rc = read_status(ctx);
	if(rc) return rc;
	return apply_status(ctx, counts);
}
// the host's half of a synchronisation, once the status block is in h_status
static int apply_status(mpm_ctx* ctx, mpm_counts* counts) {
	int rc = check_status(ctx);
	if(rc) return rc;
	ctx->pbc = ctx->h_status[ST_PBC];
	ctx->nbc = ctx->h_status[ST_NBC];
	ctx->ebc = ctx->h_status[ST_EBC];
	ctx->pbc_prev = ctx->h_status[ST_PBCPREV];
	ctx->streak_seen = ctx->h_status[ST_STREAK];
	if(ctx->ebc > ctx->g.cap) return fail(ctx, MPM_ERR_CAPACITY, "Too much exterior blocks: " + std::to_string(ctx->ebc));
	for(size_t mi = 0; mi < ctx->models.size(); ++mi) {
		Model& m	   = ctx->models[mi];
		m.bincount_src = ctx->h_status[ST_BINSPREV + mi];
		m.bincount	   = ctx->h_status[ST_BINS0 + mi];
		m.bucketed	   = ctx->h_status[ST_PART0 + mi];
		if((size_t) m.bincount > m.bin_cap) return fail(ctx, MPM_ERR_CAPACITY, "bin capacity exceeded");
	}
	if(ctx->h_status[ST_NONFINITE]) return fail(ctx, MPM_ERR_NONFINITE, "Maximum velocity is infinity");// gmpm_simulator.cuh:355-358
	rc = check_books(ctx);
	if(rc) return rc;
	rc = grow_capacity(ctx);
	if(rc) return rc;
	if(counts) return mpm_get_counts(ctx, counts);
	return MPM_OK;
}
// a rebuild of its own with its host synchronisation, timed between ev.start and ev.end (mpm_rebuild_partition, the tail of mpm_substep)
static int rebuild_and_sync(mpm_ctx* ctx, const SubstepPlan& plan, mpm_counts* counts) {
	hipStream_t s = ctx->s_compute;
	HIP_TRY(hipEventRecord(ctx->ev.start, s));
	int rc = launch_rebuild(ctx, plan, nullptr);
	if(rc) return rc;
	HIP_TRY(hipEventRecord(ctx->ev.end, s));
	HIP_TRY(hipGetLastError());
	roll_partition(ctx);
	rc = sync_counts(ctx, counts);
	if(rc) return rc;
	HIP_TRY(hipEventElapsedTime(&ctx->timers.partition_ms, ctx->ev.start, ctx->ev.end));
	return MPM_OK;
}

int mpm_rebuild_partition(mpm_ctx* ctx, mpm_counts* counts) {
	phase_call(ctx);
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	return rebuild_and_sync(ctx, default_plan(ctx), counts);
}

// Particle emission (mpm_particle_emit.hpp): a re-lay at a substep boundary.  PHASE 1 reads the context and writes scratch alone - every
// live particle gathered into staging columns, the new ones appended and checked, the merged set's partition built in a scratch table and counted - so
// that every refusal leaves the context as it was.  PHASE 2 grows what has to grow, then lays the merged columns out with set-up's own kernels
// (lay_model_bins, launch_prepare), carries the old grid over by block key and rasterises the new particles on top.
namespace {
struct EmitColumns {
	DevBuf<float> xyz, state9, logjp;
	DevBuf<int> ids;
	bool tracked = false;
	size_t live = 0, total = 0;
	EmitStage view() const { return EmitStage {xyz.p, state9.p, logjp.p, tracked ? ids.p : nullptr}; }
};
// The partition of a staged particle set, in a scratch table with a status block of its own
struct ScratchPartition {
	Partition S;
	DevBuf<int> status;
	GridCfg sg {};
	int pbc = 0, nbc = 0, ebc = 0;
};
}// namespace
// What emission and removal (mpm_particle_remove.hpp) share of the re-lay: the staging allocations' refusal, the scratch partition, the per-block
// counts, the installation of partition and bins, the books.  Each launches what mpm_emit_particles launched at that place, in that order.
static int relay_no_memory(mpm_ctx* ctx, const std::string& who, hipError_t e) {
	return e == hipSuccess ? 0 : fail(ctx, MPM_ERR_CAPACITY, who + ": no device memory for the staging arrays (" + hipGetErrorString(e) + ")");
}
#define RELAY_ALLOC(expr)                                       \
	do {                                                        \
		if(int rc_ = relay_no_memory(ctx, who, expr)) return rc_; \
	} while(0)
static int relay_alloc_columns(mpm_ctx* ctx, const std::string& who, EmitColumns& c) {
	hipStream_t s = ctx->s_compute;
	RELAY_ALLOC(c.xyz.alloc(3 * c.total, s));
	RELAY_ALLOC(c.state9.alloc(9 * c.total, s));
	RELAY_ALLOC(c.logjp.alloc(c.total, s));
	if(c.tracked) RELAY_ALLOC(c.ids.alloc(c.total, s));
	return MPM_OK;
}
// PHASE 1: the partition of the staged set (the three kernels are set-up's, in set-up's order); refuses a block capacity that does not suffice with grow = 0
static int relay_scratch_partition(mpm_ctx* ctx, const std::string& who, const std::vector<EmitColumns>& cols, size_t total_particles, ScratchPartition& P) {
	hipStream_t s	   = ctx->s_compute;
	const size_t nm	   = cols.size();
	const size_t table = (size_t) ctx->g.G * ctx->g.G * ctx->g.G;
	Partition& S	   = P.S;
	GridCfg& sg		   = P.sg;
	sg				   = ctx->g;
	int pbc			   = 0;
	RELAY_ALLOC(S.table.alloc(table, s));
	RELAY_ALLOC(S.count.alloc(1, s));
	RELAY_ALLOC(P.status.alloc(ST_WORDS, s));
	HIP_TRY(hipMemsetAsync(S.table, 0xff, sizeof(int) * table, s));
	size_t prov = std::min(table, total_particles + 1);
	RELAY_ALLOC(S.keys.alloc(3 * prov, s));
	sg.cap = (int) prov;
	for(size_t mi = 0; mi < nm; ++mi)
		if(cols[mi].total) activate_blocks_kernel<<<cdiv(cols[mi].total, 256), 256, 0, s>>>(sg, cols[mi].total, cols[mi].xyz, S.table, S.keys, S.count, P.status);
	HIP_TRY(hipMemcpyAsync(&pbc, S.count, sizeof(int), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if((size_t) pbc * 27 > prov) {// the scratch list holds every block that can be registered
		prov = std::min(table, (size_t) pbc * 27 + 1);
		RELAY_ALLOC(S.keys.grow(3 * prov, s));
		sg.cap = (int) prov;
	}
	int* st = P.status;
	HIP_TRY(hipMemcpyAsync(&st[ST_CNT_P], S.count, sizeof(int), hipMemcpyDeviceToDevice, s));
	register_blocks_kernel<0, 1><<<std::max(1u, std::min(4096u, cdiv((size_t) pbc * 8, 256))), 256, 0, s>>>(sg, &st[ST_CNT_P], nullptr, &st[ST_CNT_N], &st[ST_PBC], S.table, S.keys, st, 0);
	register_blocks_kernel<-1, 1><<<std::max(1u, std::min(8192u, cdiv((size_t) pbc * 32, 256))), 256, 0, s>>>(sg, &st[ST_CNT_P], &st[ST_CNT_N], &st[ST_CNT_E], &st[ST_NBC], S.table, S.keys, st, 0);
	int hs[ST_WORDS];
	HIP_TRY(hipMemcpyAsync(hs, st, sizeof(hs), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	if(hs[ST_OVERFLOW]) return fail(ctx, MPM_ERR_INTERNAL, who + ": the scratch partition overflowed");
	P.pbc = pbc;
	P.nbc = hs[ST_NBC];
	P.ebc = hs[ST_CNT_P] + hs[ST_CNT_N] + hs[ST_CNT_E];
	if(P.ebc > ctx->g.cap && !ctx->cfg.grow) return fail(ctx, MPM_ERR_CAPACITY, who + ": " + std::to_string(P.ebc) + " blocks needed, block capacity " + std::to_string(ctx->g.cap) + " (grow = 0)");
	return MPM_OK;
}
// PHASE 1: per model and block of the scratch partition how many particles (counts), per model how many bins; d_flags[0] takes emit_count_kernel's flags
static int relay_count_bins(mpm_ctx* ctx, const std::string& who, const std::vector<EmitColumns>& cols, const ScratchPartition& P, std::vector<DevBuf<int>>& counts, std::vector<int>& bins, int* d_flags) {
	hipStream_t s	= ctx->s_compute;
	const size_t nm = cols.size();
	const int pbc	= P.pbc;
	DevBuf<int> d_bins;
	RELAY_ALLOC(d_bins.alloc(nm, s));
	for(size_t mi = 0; mi < nm; ++mi) {
		RELAY_ALLOC(counts[mi].alloc((size_t) pbc + 1, s));
		if(!cols[mi].total) continue;
		emit_count_kernel<<<cdiv(cols[mi].total, 256), 256, 0, s>>>(P.sg, cols[mi].total, cols[mi].xyz, P.S.table, counts[mi], d_flags);
		emit_bins_kernel<<<cdiv(pbc, 256), 256, 0, s>>>(pbc, counts[mi], d_bins + mi);
	}
	int flag = 0;
	HIP_TRY(hipMemcpyAsync(&flag, d_flags, sizeof(int), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(bins.data(), d_bins, sizeof(int) * nm, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	if(flag & kEmitOutside) return fail(ctx, MPM_ERR_INTERNAL, who + ": a gathered particle has no block");
	// (as at set-up: a block that starts with more particles than it has list slots is refused whatever the overflow policy)
	if(flag & kEmitBlockFull) return fail(ctx, MPM_ERR_CAPACITY, who + ": a block would hold more than max_ppc*64 = " + std::to_string(ctx->g.ppb) + " particles");
	for(size_t mi = 0; mi < nm; ++mi)
		if((size_t) bins[mi] > ctx->models[mi].bin_cap && !ctx->cfg.grow)
			return fail(ctx, MPM_ERR_CAPACITY, who + ": model " + std::to_string(mi) + " needs " + std::to_string(bins[mi]) + " bins, bin capacity " + std::to_string(ctx->models[mi].bin_cap) + " (grow = 0)");
	return MPM_OK;
}
// PHASE 2: the scratch partition into both rolls (previous numbering == current numbering, as set-up leaves it), the counts the kernels read, and
// every model's staged columns laid out with set-up's kernels (lay_model_bins)
static int relay_install(mpm_ctx* ctx, const std::vector<EmitColumns>& cols, const ScratchPartition& P, const std::vector<int>& bins) {
	hipStream_t s	   = ctx->s_compute;
	const size_t nm	   = cols.size();
	const size_t table = (size_t) ctx->g.G * ctx->g.G * ctx->g.G;
	const GridCfg& g   = ctx->g;
	const int pbc = P.pbc, nbc = P.nbc, ebc = P.ebc;
	ctx->pbc = pbc, ctx->nbc = nbc, ctx->ebc = ebc, ctx->pbc_prev = pbc;
	{
		HIP_TRY(hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(int) * ST_WORDS, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		int* st	   = ctx->h_status;
		st[ST_PBC] = pbc, st[ST_NBC] = nbc, st[ST_EBC] = ebc, st[ST_PBCPREV] = pbc;
		st[ST_CNT_P] = st[ST_CNT_N] = st[ST_CNT_E] = 0;
		for(size_t mi = 0; mi < (size_t) kMaxModels; ++mi) {
			st[ST_BINS0 + mi]	 = 0;// (init_bins_kernel hands the bins out from here)
			st[ST_BINSPREV + mi] = mi < nm ? bins[mi] : 0;
			st[ST_PART0 + mi]	 = mi < nm ? (int) cols[mi].total : 0;
		}
		HIP_TRY(hipMemcpyAsync(ctx->d_status, st, sizeof(int) * ST_WORDS, hipMemcpyHostToDevice, s));
		for(int i = 0; i < 2; ++i) {
			HIP_TRY(hipMemcpyAsync(ctx->part[i].table, P.S.table, sizeof(int) * table, hipMemcpyDeviceToDevice, s));
			HIP_TRY(hipMemcpyAsync(ctx->part[i].keys, P.S.keys, sizeof(int) * 3 * (size_t) ebc, hipMemcpyDeviceToDevice, s));
			HIP_TRY(hipMemcpyAsync(ctx->part[i].count, &st[ST_EBC], sizeof(int), hipMemcpyHostToDevice, s));
		}
		HIP_TRY(hipStreamSynchronize(s));
	}
	for(size_t mi = 0; mi < nm; ++mi) {
		Model& m = ctx->models[mi];
		HIP_TRY(hipMemsetAsync(m.size, 0, sizeof(int) * ((size_t) g.cap + 1), s));
		HIP_TRY(hipMemsetAsync(m.out_count, 0, sizeof(int) * ((size_t) g.cap + 1), s));
		if(m.pair)
			for(int i = 0; i < 2; ++i) HIP_TRY(hipMemsetAsync(m.pairinfo[i], 0, sizeof(int) * ((size_t) g.cap + 1) * kPairChunks, s));
		const EmitColumns& c = cols[mi];
		ParticleInit staged;
		staged.state9 = c.state9, staged.logjp = c.logjp;
		if(int rc = lay_model_bins(ctx, mi, P.S.table, pbc, {c.total, c.xyz, staged, true, c.tracked ? c.ids.p : nullptr})) return rc;
	}
	return MPM_OK;
}
// PHASE 2, after launch_prepare and read_status: every model's bins and bucketed count as the re-lay left them
static int relay_books(mpm_ctx* ctx, const std::string& who, const std::vector<EmitColumns>& cols, const std::vector<int>& bins) {
	for(size_t mi = 0; mi < cols.size(); ++mi) {
		Model& m	   = ctx->models[mi];
		m.bincount	   = ctx->h_status[ST_BINS0 + mi];
		m.bincount_src = m.bincount;
		m.bucketed	   = (int64_t) cols[mi].total;
		if(m.bincount != bins[mi]) return fail(ctx, MPM_ERR_INTERNAL, who + ": model " + std::to_string(mi) + " took " + std::to_string(m.bincount) + " bins, " + std::to_string(bins[mi]) + " were counted");
	}
	return MPM_OK;
}
int mpm_emit_particles(mpm_ctx* ctx, int model, const float* xyz, size_t n, const float v0[3], const mpm_particle_init* init, int32_t* first_id) {
	if(!ctx) return MPM_ERR_INVALID;
	const std::string who = "mpm_emit_particles";
	if(!ctx->ready) return fail(ctx, MPM_ERR_NOT_READY, who + ": particles are emitted after mpm_initial_setup (before it, add them with the model)");
	if(model < 0 || model >= (int) ctx->models.size()) return fail(ctx, MPM_ERR_INVALID, who + ": no model " + std::to_string(model));
	if(!xyz && n) return fail(ctx, MPM_ERR_INVALID, who + ": positions are missing");
	if(init) {
		for(int r: init->reserved)
			if(r) return fail(ctx, MPM_ERR_INVALID, who + ": a reserved word of mpm_particle_init is not 0");
		if(init->state9 && init->state_kind != MPM_STATE_B && init->state_kind != MPM_STATE_F)
			return fail(ctx, MPM_ERR_INVALID, who + ": unknown state_kind " + std::to_string(init->state_kind) + " (MPM_STATE_B or MPM_STATE_F)");
	}
	VelocityField f {};
	for(int d = 0; d < 3; ++d) {
		f.v0[d] = v0 ? v0[d] : 0.f;
		if(!std::isfinite(f.v0[d])) return fail(ctx, MPM_ERR_INVALID, who + ": v0 is not finite");
	}
	if(ctx->group_refs > 0 || ctx->mgsp_rank >= 0 || ctx->halo_tagged || ctx->d_overlap.p)// (the halo arrays outlive a tagging that a checkpoint load has made stale)
		return fail(ctx, MPM_ERR_INVALID, who + ": the context belongs (or belonged) to a multi-GPU group or has been through the halo tagging; emission into groups is not computed");
	if(!ctx->grid_momentum || ctx->grid_preupdated)
		return fail(ctx, MPM_ERR_INVALID, who + ": the grid holds velocities (a grid update without its rebuild): emit at a substep boundary");
	if(ctx->track_ids && !ctx->ids_valid) return fail(ctx, MPM_ERR_INVALID, who + ": the ids are not valid (load them with mpm_particle_ids_load first)");
	Model& M = ctx->models[model];
	if(M.n + n > (size_t) 0x7fffffff) return fail(ctx, MPM_ERR_CAPACITY, who + ": a model holds at most 2^31 - 1 particles");
	const int32_t old_n = (int32_t) M.n;
	if(n == 0) {
		if(first_id) *first_id = old_n;
		return MPM_OK;
	}
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	hipStream_t s		= ctx->s_compute;
	const size_t nm		= ctx->models.size();
	const size_t table	= (size_t) ctx->g.G * ctx->g.G * ctx->g.G;
	const bool fluid	= M.material == MPM_J_FLUID;
	// ---- phase 1: gather, append, check, count - the context is only read ----
	std::vector<EmitColumns> cols(nm);
	DevBuf<unsigned long long> d_gathered;
	DevBuf<int> d_flags;// [0] emission's own, [1] validate_particle_init_kernel's
	RELAY_ALLOC(d_gathered.alloc(nm, s));
	RELAY_ALLOC(d_flags.alloc(2, s));
	size_t total_particles = 0;
	for(size_t mi = 0; mi < nm; ++mi) {
		const Model& m = ctx->models[mi];
		EmitColumns& c = cols[mi];
		c.live		   = (size_t) m.bucketed;
		c.total		   = c.live + ((int) mi == model ? n : 0);
		c.tracked	   = ctx->track_ids;
		total_particles += c.total;
		if(int rc = relay_alloc_columns(ctx, who, c)) return rc;
		if(c.live && ctx->pbc) emit_gather_kernel<<<ctx->pbc, kReadoutThreads, 0, s>>>(make_readout_args(ctx, m), c.view(), (unsigned long long) c.live, d_gathered + mi);
	}
	EmitColumns& E = cols[model];
	HIP_TRY(hipMemcpyAsync(E.xyz + 3 * E.live, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, s));
	DevBuf<float> d_velocity, d_affine, d_state, d_logjp;
	ParticleInit a;
	if(init) {
		const bool with_logjp = init->logjp && (M.material == MPM_SAND || M.material == MPM_NACC);// (ignored where the material has no log Jp)
		struct {
			const float* host;
			DevBuf<float>* dev;
			const float** view;
			size_t per;
		} up[4] = {{init->velocity, &d_velocity, &a.velocity, 3}, {init->affine9, &d_affine, &a.affine9, 9}, {init->state9, &d_state, &a.state9, 9}, {with_logjp ? init->logjp : nullptr, &d_logjp, &a.logjp, 1}};
		for(auto& c: up) {
			if(!c.host) continue;
			RELAY_ALLOC(c.dev->alloc(c.per * n, s));
			HIP_TRY(hipMemcpyAsync(c.dev->p, c.host, sizeof(float) * c.per * n, hipMemcpyHostToDevice, s));
			*c.view = c.dev->p;
		}
		a.state_f = init->state9 && init->state_kind == MPM_STATE_F ? 1 : 0;
		if(a.velocity || a.affine9 || a.state9 || a.logjp) validate_particle_init_kernel<<<std::min(4096u, cdiv(n, 256)), 256, 0, s>>>(n, fluid, a, d_flags + 1);
	}
	emit_append_kernel<<<std::min(4096u, cdiv(n, 256)), 256, 0, s>>>(ctx->g, n, E.live, fluid, M.mc.log_jp0, old_n, a, E.view(), d_flags);
	{
		std::vector<unsigned long long> gathered(nm);
		int flags[2] = {0, 0};
		HIP_TRY(hipMemcpyAsync(gathered.data(), d_gathered, sizeof(unsigned long long) * nm, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(s));
		for(size_t mi = 0; mi < nm; ++mi)
			if(gathered[mi] != cols[mi].live)
				return fail(ctx, MPM_ERR_INTERNAL, who + ": the lists of model " + std::to_string(mi) + " hold " + std::to_string(gathered[mi]) + " particles, the books " + std::to_string(cols[mi].live));
		if(flags[0] & kEmitBadPosition) return fail(ctx, MPM_ERR_INVALID, who + ": xyz holds a value that is not finite");
		if(flags[0] & kEmitOutside) return fail(ctx, MPM_ERR_INVALID, who + ": particles outside the domain");
		if(flags[1] & kInitBadVelocity) return fail(ctx, MPM_ERR_INVALID, who + ": velocity holds a value that is not finite");
		if(flags[1] & kInitBadAffine) return fail(ctx, MPM_ERR_INVALID, who + ": affine9 holds a value that is not finite");
		if(flags[1] & kInitBadState) return fail(ctx, MPM_ERR_INVALID, who + ": state9 holds a value that is not finite");
		if(flags[1] & kInitBadLogJp) return fail(ctx, MPM_ERR_INVALID, who + ": logjp holds a value that is not finite");
		if(flags[1] & kInitNotPositive) return fail(ctx, MPM_ERR_INVALID, who + (fluid ? ": state9 holds a J that is not strictly positive" : ": state9 holds a |b00|, b11 or b22 that is not strictly positive"));
	}
	// the partition of the merged set, in a scratch table with a status block of its own; per model and block: how many particles, how many bins
	ScratchPartition SP;
	if(int rc = relay_scratch_partition(ctx, who, cols, total_particles, SP)) return rc;
	const int pbc = SP.pbc, nbc = SP.nbc, ebc = SP.ebc;
	const bool grow = ctx->cfg.grow != 0;
	std::vector<DevBuf<int>> counts(nm);
	std::vector<int> bins(nm, 0);
	if(int rc = relay_count_bins(ctx, who, cols, SP, counts, bins, d_flags)) return rc;
	// the old grid and its keys, kept aside
	const int r = ctx->rollid, old_nbc = ctx->nbc;
	DevBuf<float> old_grid;
	DevBuf<int> old_keys;
	RELAY_ALLOC(old_grid.alloc(256 * (size_t) old_nbc, s));
	RELAY_ALLOC(old_keys.alloc(3 * (size_t) old_nbc, s));
	HIP_TRY(hipMemcpyAsync(old_grid, ctx->grid[0], sizeof(float) * 256 * (size_t) old_nbc, hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipMemcpyAsync(old_keys, ctx->part[r].keys, sizeof(int) * 3 * (size_t) old_nbc, hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipStreamSynchronize(s));
	// ---- phase 2: nothing refuses from here on.  Capacities first (the growth policy's steps; every array keeps what it holds) ----
	phase_call(ctx);
	while(ebc > ctx->g.cap)
		if(int rc = reserve_blocks(ctx, std::min(table, (size_t) ctx->g.cap * 3 / 2 + 1))) return rc;
	const size_t new_n = M.n + n;
	for(size_t mi = 0; mi < nm; ++mi) {
		Model& m		  = ctx->models[mi];
		const size_t need = std::max((size_t) bins[mi], grow ? ((int) mi == model ? new_n : m.n) / kBin + (size_t) ctx->g.cap + 1 : 0);
		if(need > m.bin_cap)// (by the policy's 3/2 at the least: a tap emits layer after layer and must not regrow its bins for every one)
			if(int rc = reserve_bins(ctx, m, std::max(need, m.bin_cap * 3 / 2 + 1))) return rc;
	}
	HIP_TRY(M.d_xyz.grow(3 * new_n, s));
	const GridCfg& g = ctx->g;
	// the partition, in both rolls, the counts the kernels read, and every model's columns into bins
	if(int rc = relay_install(ctx, cols, SP, bins)) return rc;
	// the grid: zero, the old blocks under their new numbers, the new particles on top (set-up's P2G of them alone; M.list[1] is free again)
	HIP_TRY(hipMemsetAsync(ctx->grid[0], 0, sizeof(float) * 256 * (size_t) nbc, s));
	HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int) * 2, s));
	if(old_nbc) emit_carry_grid_kernel<<<std::min(2048u, cdiv(old_nbc, 4)), 256, 0, s>>>(g, old_nbc, nbc, old_keys, old_grid, ctx->part[r].table, ctx->grid[0], d_flags);
	{
		int* fresh = counts[model];
		HIP_TRY(hipMemsetAsync(fresh, 0, sizeof(int) * ((size_t) pbc + 1), s));
		const float* nxyz = E.xyz + 3 * E.live;
		bucket_particles_kernel<<<cdiv(n, 256), 256, 0, s>>>(g, n, nxyz, ctx->part[r].table, fresh, M.list[1], SP.status);
		rasterize_particles_kernel<false><<<pbc, 256, 0, s>>>(g, nxyz, M.list[1], fresh, ctx->part[r].keys, ctx->part[r].table, ctx->grid[0], M.mc.mass, a, f);
	}
	int rc = launch_prepare(ctx, PrepareFor::Setup);
	if(rc) return rc;
	HIP_TRY(hipGetLastError());
	rc = read_status(ctx);
	if(rc) return rc;
	{
		int flag = 0;
		HIP_TRY(hipMemcpy(&flag, d_flags, sizeof(int), hipMemcpyDeviceToHost));
		if(flag & kEmitCarryMiss) return fail(ctx, MPM_ERR_INTERNAL, who + ": a block of the old grid has no number in the new partition");
	}
	// the books
	M.n = new_n;
	if(int rc2 = relay_books(ctx, who, cols, bins)) return rc2;
	ctx->relaid = true;
	if(first_id) *first_id = old_n;
	return grow_capacity(ctx);// (the policy's own look at the new fill levels)
}

int mpm_substep(mpm_ctx* ctx, float dt, float step_time, float frame_time, float dt_default, float* next_dt, float* max_vel) {
	phase_call(ctx);
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	FlagGuard guard {ctx};
	float mv2 = 0.f;
	int rc	  = mpm_grid_update(ctx, dt, &mv2);
	if(rc) return rc;
	if(std::isinf(mv2)) return fail(ctx, MPM_ERR_NONFINITE, "Maximum velocity is infinity");// gmpm_simulator.cuh:355-358
	const float mv = std::sqrt(mv2);																 // :360
	const float nd = mpm_compute_dt(ctx, mv, step_time, frame_time, dt_default);
	if(max_vel) *max_vel = mv;
	if(next_dt) *next_dt = nd;
	SubstepPlan plan   = default_plan(ctx, dt, nd);// (this path keeps the grid update a kernel of its own: no fuse_dt)
	plan.rebuild_clear = true;
	if((rc = launch_g2p2g(ctx, plan)) || (rc = rebuild_and_sync(ctx, plan, nullptr))) return rc;
	HIP_TRY(hipEventElapsedTime(&ctx->last_g2p2g_ms, ctx->ev.g2p2g_start, ctx->ev.g2p2g_end));
	ctx->timers.g2p2g_ms = ctx->last_g2p2g_ms;
	ctx->timers.total_ms = ctx->timers.grid_update_ms + ctx->timers.g2p2g_ms + ctx->timers.partition_ms;
	guard.armed = false;
	return MPM_OK;
}

// The substep loop with fixed dt.  The host enqueues up to mpm_config.sync_interval substeps (default 8) back to back and only
// then synchronises: every kernel reads its block counts from the status block, launches are sized by the counts of the last
// synchronisation plus a margin (a kernel walks over what is beyond its launch), errors raised in between are sticky flags.
// The reference synchronises the host six times per substep (gmpm_simulator.cuh:398,:470,:503,:518,:541,:564).
int mpm_run_fixed(mpm_ctx* ctx, int nsteps, float dt) {
	phase_call(ctx);
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	const int K = ctx->cfg.sync_interval > 0 ? std::min(ctx->cfg.sync_interval, 64) : 8;// (clamped to 64: claymore_amd.h)
	FlagGuard guard {ctx};
	const bool still_on = ctx->cfg.still_rebuild != -1 && ctx->group_refs == 0;// (a grouped context's rebuilds belong to the group loop)
	while((int) ctx->ev_ring.size() < 3 * K + 1) {
		hipEvent_t e = nullptr;
		HIP_TRY(hipEventCreate(&e));
		ctx->ev_ring.push_back(e);
	}
	{// the counts are exact here: a context that starts a run above the 3/4 mark grows before its first window, not after it
		int rc = grow_capacity(ctx);
		if(rc) return rc;
	}
	double acc_grid = 0, acc_g2p2g = 0, acc_part = 0, acc_total = 0;
	int in_window = 0;
	// Where a substep's four times come from.  STAMPS (the default): the kernels that open its phases write the wall clock into the substep's row of the ring behind
	// the status block (mpm_kernels.hpp: phase_stamp) - substep_clear_kernel, its first launch, the start; G2P2G's first launch and compact_blocks_kernel the
	// phase boundaries; its end is the next row's start, written by the next substep's clear or, behind the last substep of a window, by a one-thread launch -
	// and the rows come back with the window's status read-back: nothing is put on the stream for the timers but that one launch per window.  EVENTS
	// (MPM_PHASE_TIMERS=events: every substep; otherwise the substep that launches the stand-alone grid update - the first of a call - and a context without
	// particle blocks, whose G2P2G launches nothing): three per substep - start, G2P2G start, G2P2G end -, its end is the next substep's start or an event
	// of its own.  An event between two kernels is a barrier packet of its own, 5-6 us on the stream (profiles/r06_rank_alone_seq.txt).
	bool stamped[64] = {};// per substep of the window
	bool open_row	 = false;// the previous substep of this window was stamped and nobody has written its end yet
	auto close_row = [&]() {// the end of the window's substep in_window - 1 = the start of row in_window
		if(open_row) phase_stamp_kernel<<<1, 1, 0, s>>>(ctx->d_stamps + (size_t) in_window * kStampRow);
		open_row = false;
	};
	const double ms_per_tick = ctx->wall_clock_khz > 0 ? 1.0 / ctx->wall_clock_khz : 0.0;
	for(int it = 0; it < nsteps; ++it) {
		const bool by_stamps = !ctx->phase_events && ctx->grid_preupdated && ctx->pbc > 0;
		stamped[in_window]	 = by_stamps;
		hipEvent_t* ev		 = &ctx->ev_ring[3 * in_window];
		SubstepPlan plan {dt, dt};
		plan.offer_still = still_on, plan.rebuild_clear = true;
		// the last substep leaves the canonical state behind; the load gauge reads every update's momenta first; a rigid body's update is a kernel of its own;
		// the force fields' pass runs ahead of a stand-alone update
		if(it + 1 < nsteps && !ctx->load_gauge && !ctx->body_mask && !ctx->force.count) plan.fuse_dt = dt;
		if(by_stamps)
			plan.stamp_row = ctx->d_stamps + (size_t) in_window * kStampRow;// (its clear writes the previous substep's end)
		else {
			plan.ev.g2p2g_start = ev[1], plan.ev.g2p2g_end = ev[2];
			close_row();
			if(in_window == 0 || stamped[in_window - 1]) HIP_TRY(hipEventRecord(ev[0], s));
		}
		int rc = launch_grid_update(ctx, dt);
		if(rc || (rc = launch_g2p2g(ctx, plan)) || (rc = launch_rebuild(ctx, plan, nullptr))) return rc;
		if(!by_stamps) HIP_TRY(hipEventRecord(ev[3], s));
		open_row = by_stamps;
		roll_partition(ctx);
		++in_window;
		// Capacities grow only at a synchronisation (by 3/2 per look, at 3/4 fill): a context whose blocks fill more than 7/10 of the capacity
		// (set-up sizes it to 2/3) looks after EVERY substep - what the reference's check_capacity does (gmpm_simulator.cuh:283-300) -,
		// so that a burst of new blocks cannot outrun the growth inside a window
		const bool tight = ctx->cfg.grow && (long long) ctx->ebc * 10 > (long long) ctx->g.cap * 7 &&
						   (size_t) ctx->g.cap < (size_t) ctx->g.G * ctx->g.G * ctx->g.G;// (a capacity that has reached the table size cannot grow: nothing to look for)
		if(in_window == K || it + 1 == nsteps || tight) {
			close_row();
			HIP_TRY(hipGetLastError());
			rc = sync_counts(ctx, nullptr);// (one read-back: status, halo counters, max |v|^2 slots, phase stamps)
			if(rc) return rc;
			if(std::isinf(host_maxvel(ctx))) return fail(ctx, MPM_ERR_NONFINITE, "Maximum velocity is infinity");
			for(int w = 0; w < in_window; ++w) {
				float t_grid = 0, t_g = 0, t_part = 0, t_tot = 0;
				if(stamped[w]) {
					const unsigned long long* r = ctx->h_stamps + (size_t) w * kStampRow;
					const unsigned long long t0 = r[0], t1 = r[1], t2 = r[2], t3 = r[kStampRow];
					auto ms = [&](unsigned long long a, unsigned long long b) { return b > a ? (float) ((double) (b - a) * ms_per_tick) : 0.f; };
					t_grid = ms(t0, t1), t_g = ms(t1, t2), t_part = ms(t2, t3), t_tot = ms(t0, t3);
				} else {
					hipEvent_t* e = &ctx->ev_ring[3 * w];
					HIP_TRY(hipEventElapsedTime(&t_grid, e[0], e[1]));
					HIP_TRY(hipEventElapsedTime(&t_g, e[1], e[2]));
					HIP_TRY(hipEventElapsedTime(&t_part, e[2], e[3]));
					HIP_TRY(hipEventElapsedTime(&t_tot, e[0], e[3]));
				}
				acc_grid += t_grid;
				acc_g2p2g += t_g;
				acc_part += t_part;
				acc_total += t_tot;
				ctx->last_g2p2g_ms = t_g;
			}
			in_window = 0;
		}
	}
	if(nsteps > 0) {// per-substep averages over this call, on the compute stream's own time (phase stamps or HIP events, above)
		ctx->timers.grid_update_ms = (float) (acc_grid / nsteps);
		ctx->timers.g2p2g_ms	   = (float) (acc_g2p2g / nsteps);
		ctx->timers.partition_ms   = (float) (acc_part / nsteps);
		ctx->timers.total_ms	   = (float) (acc_total / nsteps);
	}
	guard.armed = false;
	return MPM_OK;
}

int mpm_state_kind(void) {
	return MPM_STATE_B;
}

const char* mpm_build_info(void) {
	return "claymore_hip abi7 state=b"
#ifdef MPM_EXPERIMENT
		   " experiment=MPM_EXPERIMENT"
#ifdef MPM_HACK_STALE_INTERIOR
		   ",MPM_HACK_STALE_INTERIOR"
#endif
#ifdef MPM_G2P2G_STATS
		   ",MPM_G2P2G_STATS"
#endif
#else
		   " experiment=none"
#endif
		;
}

int mpm_last_g2p2g_ms(mpm_ctx* ctx, float* ms) {
	if(!ctx || !ms) return MPM_ERR_INVALID;
	*ms = ctx->last_g2p2g_ms;
	return MPM_OK;
}

int mpm_still_launch_sizes(const char* setting, int streak, int still_on, int particle_blocks, int* prepare_workgroups, int* register_workgroups) {
	if(!prepare_workgroups || !register_workgroups) return MPM_ERR_INVALID;
	const StillLaunch t	 = still_launch_rule(streak, still_on != 0, particle_blocks, still_launch_override(setting));
	*prepare_workgroups	 = t.prepare;
	*register_workgroups = t.reg;
	return MPM_OK;
}

int mpm_get_counts(mpm_ctx* ctx, mpm_counts* counts) {
	if(!ctx || !ctx->ready || !counts) return MPM_ERR_NOT_READY;
	memset(counts, 0, sizeof(*counts));
	counts->particle_blocks = ctx->pbc;
	counts->neighbor_blocks = ctx->nbc;
	counts->exterior_blocks = ctx->ebc;
	counts->model_count		= (int) ctx->models.size();
	for(size_t mi = 0; mi < ctx->models.size(); ++mi) {
		counts->bins[mi]	  = ctx->models[mi].bincount;
		counts->particles[mi] = ctx->models[mi].bucketed;
	}
	return MPM_OK;
}

int mpm_default_collision_object(mpm_collision_object* o) {
	if(!o) return MPM_ERR_INVALID;
	memset(o, 0, sizeof(*o));
	o->type		  = MPM_BOUNDARY_STICKY;// boundary_condition.cuh:43-48
	o->friction	  = 0.3f;
	o->scale	  = 1.0f;
	o->dsdt		  = 0.0f;
	o->rot_mat[0] = o->rot_mat[4] = o->rot_mat[8] = 1.f;
	return MPM_OK;
}

// the two range checks every collider install makes (the messages carry the API's prefix, so they stay with the callers)
static bool boundary_type_ok(const mpm_collision_object* obj) {
	return obj->type >= MPM_BOUNDARY_STICKY && obj->type <= MPM_BOUNDARY_SEPARATE;
}
static bool slot_ok(int slot) {
	return slot >= 0 && slot < MPM_MAX_COLLISION_SHAPES;
}
// the pose, motion and boundary fields of mpm_collision_object as the kernels read them (no field: a slot's collider)
static CollisionObject slot_object(const mpm_collision_object* obj) {
	CollisionObject o {};
	o.type	   = obj->type;
	o.friction = obj->friction;
	o.scale	   = obj->scale;
	o.dsdt	   = obj->dsdt;
	for(int d = 0; d < 3; ++d) o.trans[d] = obj->trans[d], o.trans_vel[d] = obj->trans_vel[d], o.omega[d] = obj->omega[d];
	for(int i = 0; i < 9; ++i) o.rot[i] = obj->rot_mat[i];
	o.time	= obj->time;
	o.field = nullptr;
	return o;
}

int mpm_set_collision_object(mpm_ctx* ctx, const mpm_collision_object* obj, const float* sdf, const float* gx, const float* gy, const float* gz) {
	if(!ctx) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(ctx->d_sdf.reset());
	ctx->has_collision	   = false;
	ctx->collision_running = false;// installing or removing an object stops the clock
	if(!obj) return MPM_OK;
	if(!sdf || !gx || !gy || !gz) return fail(ctx, MPM_ERR_INVALID, "collision object without a signed distance field");
	if(!boundary_type_ok(obj)) return fail(ctx, MPM_ERR_INVALID, "[ERROR] Wrong Boundary Type!");// boundary_condition.cuh:244
	const size_t N = (size_t) 1 << ctx->cfg.domain_bits, n = N * N * N;
	DevBuf<float> stage;
	HIP_TRY(stage.alloc(4 * n, ctx->s_compute));
	HIP_TRY(ctx->d_sdf.alloc(n, ctx->s_compute));
	const float* src[4] = {sdf, gx, gy, gz};
	for(int c = 0; c < 4; ++c) HIP_TRY(hipMemcpy(stage + c * n, src[c], sizeof(float) * n, hipMemcpyHostToDevice));
	pack_sdf_kernel<<<cdiv(n, 256), 256, 0, ctx->s_compute>>>(n, stage, stage + n, stage + 2 * n, stage + 3 * n, ctx->d_sdf);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(ctx->s_compute));
	HIP_TRY(stage.reset());
	ctx->collision		 = slot_object(obj);
	ctx->collision.field = ctx->d_sdf;
	ctx->has_collision	 = true;
	return MPM_OK;
}

// Analytic collision shapes ------------------------------------------------------------------------------------------------------------
static bool shape_finite3(const float* v) {
	return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
}
// mpm_collision_object + mpm_collision_shape -> the slot the kernels read; nullptr, or the message that names the offending field
static const char* make_shape_slot(const mpm_collision_object* obj, const mpm_collision_shape* sh, ShapeSlot& out) {
	if(sh->kind < MPM_SHAPE_HALFSPACE || sh->kind > MPM_SHAPE_CAPSULE) return "collision shape: unknown kind";
	if(!boundary_type_ok(obj)) return "collision shape: boundary type outside 0..2";
	for(int d = 0; d < 3; ++d)
		if(sh->a[d] != sh->a[d]) return "collision shape: NaN in a";
	if(sh->radius != sh->radius) return "collision shape: NaN in radius";
	if(sh->kind != MPM_SHAPE_SPHERE)
		for(int d = 0; d < 3; ++d)
			if(sh->b[d] != sh->b[d]) return "collision shape: NaN in b";
	ShapeSlot c {};
	c.shape.kind	   = sh->kind;
	c.shape.inside_out = sh->inside_out ? 1 : 0;
	for(int d = 0; d < 3; ++d) c.shape.a[d] = sh->a[d], c.shape.b[d] = sh->b[d];
	c.shape.radius = sh->radius;
	if(sh->kind == MPM_SHAPE_SPHERE || sh->kind == MPM_SHAPE_CAPSULE) {
		if(!(sh->radius > 0.f) || !std::isfinite(sh->radius)) return "collision shape: radius must be finite and > 0";
	} else
		c.shape.radius = 0.f;
	if(sh->kind == MPM_SHAPE_SPHERE) c.shape.b[0] = c.shape.b[1] = c.shape.b[2] = 0.f;
	if(sh->kind == MPM_SHAPE_HALFSPACE) {
		if(!shape_finite3(sh->b)) return "collision shape: normal b must be finite";
		const float len = sqrtf(sh->b[0] * sh->b[0] + sh->b[1] * sh->b[1] + sh->b[2] * sh->b[2]);
		if(!(len > 0.f) || !std::isfinite(len)) return "collision shape: normal b must not be zero";
		for(int d = 0; d < 3; ++d) c.shape.b[d] = sh->b[d] / len;// (a unit axis stays exactly itself)
	}
	if(sh->kind == MPM_SHAPE_BOX)
		for(int d = 0; d < 3; ++d)
			if(!(sh->b[d] > 0.f) || !std::isfinite(sh->b[d])) return "collision shape: half extents b must be finite and > 0";
	if(sh->kind == MPM_SHAPE_CAPSULE && sh->a[0] == sh->b[0] && sh->a[1] == sh->b[1] && sh->a[2] == sh->b[2]) return "collision shape: capsule end points a and b coincide";
	c.obj = slot_object(obj);
	out	  = c;
	return nullptr;
}

static void count_slots(mpm_ctx* ctx) {
	ctx->shape_count = ctx->hf_count = ctx->vol_count = 0;
	for(int i = 0; i < MPM_MAX_COLLISION_SHAPES; ++i) {
		if(ctx->shape[i].shape.kind) ctx->shape_count = i + 1;
		if(ctx->shape[i].shape.kind == kShapeHeightfield) ++ctx->hf_count;
		if(ctx->shape[i].shape.kind == kShapeVolume) ++ctx->vol_count;
	}
}
// What sits in a slot.  All empty: nothing (shape.shape.kind 0); an analytic shape fills `shape` alone; a heightfield `shape` and `hf`; a volume
// `shape`, `vol` and `desc`, its descriptor as installed; `table` is the heightfield's or the volume's (hf.table / vol.table: set by install_slot).
struct SlotOccupant {
	ShapeSlot shape {};
	Heightfield hf {};
	Volume vol {};
	mpm_collision_volume desc {};
	DevBuf<float4> table;
};
// What every accepted install or removal of any kind does to slot `slot`: wait for the device, free the table of a heightfield or a volume
// that sat there, put the new occupant in (o.table: the new heightfield's / volume's, owned by the context's slot_table from here on; a
// refused install frees it with o), stop the clock and - on an install - set it to obj->time.
static int install_slot(mpm_ctx* ctx, int slot, SlotOccupant& o, const mpm_collision_object* obj) {
	hipError_t e = hipSetDevice(ctx->device);
	if(e == hipSuccess) e = hipDeviceSynchronize();
	if(e != hipSuccess) return fail(ctx, MPM_ERR_DEVICE, std::string("collision slot: ") + hipGetErrorString(e));// nothing was touched: the old occupant stays
	// the old table goes first; should freeing it fail, its memory is in an unknown state, so the slot is emptied rather than left pointing at it
	if((e = ctx->slot_table[slot].reset()) != hipSuccess) {
		ctx->hf[slot]		= Heightfield {};
		ctx->vol[slot]		= Volume {};
		ctx->vol_desc[slot] = mpm_collision_volume {};
		ctx->shape[slot]	= ShapeSlot {};
		ctx->body_mask &= ~(1 << slot);
		ctx->frozen[slot] = false;
		count_slots(ctx);
		return fail(ctx, MPM_ERR_DEVICE, std::string("collision slot: freeing the old table -> ") + hipGetErrorString(e) + " (the slot is now empty)");
	}
	ctx->slot_table[slot] = std::move(o.table);
	ctx->hf[slot]		  = o.hf;
	ctx->vol[slot]		  = o.vol;
	if(o.shape.shape.kind == kShapeHeightfield) ctx->hf[slot].table = ctx->slot_table[slot];
	if(o.shape.shape.kind == kShapeVolume) ctx->vol[slot].table = ctx->slot_table[slot];
	ctx->vol_desc[slot]	   = o.desc;
	ctx->shape[slot]	   = o.shape;// (kind 0: empty)
	ctx->body_mask &= ~(1 << slot);// any install over a slot, or emptying it, removes its rigid body
	ctx->frozen[slot]	   = false;
	ctx->collision_running = false;// installing or removing a collider stops the clock
	if(obj) ctx->collision.time = obj->time;
	count_slots(ctx);
	return MPM_OK;
}

int mpm_set_collision_shape(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_collision_shape* shape) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!slot_ok(slot)) return fail(ctx, MPM_ERR_INVALID, "collision shape: slot outside 0..3");
	SlotOccupant o;
	if(obj) {
		if(!shape) return fail(ctx, MPM_ERR_INVALID, "collision shape: obj without a shape");
		if(const char* msg = make_shape_slot(obj, shape, o.shape)) return fail(ctx, MPM_ERR_INVALID, msg);
	}
	return install_slot(ctx, slot, o, obj);
}

// Particle removal (mpm_particle_remove.hpp): emission's mirror image, a re-lay at a substep boundary.  PHASE 1 reads the context and
// writes scratch alone - the selected particles counted (nothing selected: the call ends there), every model split into the survivors' staging columns
// and the removed list, the survivors' partition built in a scratch table and counted, the removed particles' stencil nodes marked in the old
// numbering.  PHASE 2 lays the survivors out with set-up's own kernels (relay_install), carries the old grid over by block key, rasterises the
// survivors' set-up mass into a scratch grid and rescales the marked nodes to it.
namespace {
struct SinkQuery {
	SinkSelect sel {};
	DevBuf<unsigned> bitmap;
	DevBuf<int> d_ids;
};
}// namespace
// the regions as mpm_set_collision_shape would install them (make_shape_slot: the same checks, the half-space normal normalised the same way)
static int sink_regions(mpm_ctx* ctx, const std::string& who, const mpm_collision_shape* regions, int nregions, SinkSelect& q) {
	if(nregions < 0 || nregions > MPM_MAX_SINK_REGIONS) return fail(ctx, MPM_ERR_INVALID, who + ": nregions outside 0.." + std::to_string(MPM_MAX_SINK_REGIONS));
	if(nregions && !regions) return fail(ctx, MPM_ERR_INVALID, who + ": regions are missing");
	mpm_collision_object obj;
	mpm_default_collision_object(&obj);
	for(int i = 0; i < nregions; ++i) {
		ShapeSlot slot;
		if(const char* msg = make_shape_slot(&obj, &regions[i], slot)) return fail(ctx, MPM_ERR_INVALID, who + ": region " + std::to_string(i) + ": " + msg);
		q.region[i] = slot.shape;
	}
	q.nregions = nregions;
	return MPM_OK;
}
// emission's preconditions, with emission's codes
static int sink_preconditions(mpm_ctx* ctx, const std::string& who, int model) {
	if(!ctx->ready) return fail(ctx, MPM_ERR_NOT_READY, who + ": particles are removed after mpm_initial_setup");
	if(model < -1 || model >= (int) ctx->models.size()) return fail(ctx, MPM_ERR_INVALID, who + ": no model " + std::to_string(model));
	if(ctx->group_refs > 0 || ctx->mgsp_rank >= 0 || ctx->halo_tagged || ctx->d_overlap.p)
		return fail(ctx, MPM_ERR_INVALID, who + ": the context belongs (or belonged) to a multi-GPU group or has been through the halo tagging; removal from groups is not computed");
	if(!ctx->grid_momentum || ctx->grid_preupdated)
		return fail(ctx, MPM_ERR_INVALID, who + ": the grid holds velocities (a grid update without its rebuild): remove at a substep boundary");
	if(ctx->track_ids && !ctx->ids_valid) return fail(ctx, MPM_ERR_INVALID, who + ": the ids are not valid (load them with mpm_particle_ids_load first)");
	return MPM_OK;
}
// the count pass: how many live particles of each selected model the query selects (the one thing a call that selects nothing launches)
static int sink_count(mpm_ctx* ctx, int model, const SinkQuery& q, int64_t out[8]) {
	hipStream_t s	= ctx->s_compute;
	const size_t nm = ctx->models.size();
	for(int i = 0; i < 8; ++i) out[i] = 0;
	unsigned long long found[8] = {0};
	HIP_TRY(hipMemsetAsync(ctx->d_totals, 0, sizeof(double) * 4, s));// (four 8-byte words the context owns; the models go through them four at a time)
	for(size_t first = 0; first < nm; first += 4) {
		bool any = false;
		for(size_t mi = first; mi < std::min(nm, first + 4); ++mi) {
			const Model& m = ctx->models[mi];
			if((model >= 0 && (int) mi != model) || !m.bucketed || !ctx->pbc) continue;
			sink_count_kernel<<<ctx->pbc, kReadoutThreads, 0, s>>>(make_readout_args(ctx, m), q.sel, reinterpret_cast<unsigned long long*>(ctx->d_totals.p) + (mi - first));
			any = true;
		}
		if(!any) continue;
		HIP_TRY(hipMemcpyAsync(found + first, ctx->d_totals, sizeof(unsigned long long) * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemsetAsync(ctx->d_totals, 0, sizeof(double) * 4, s));
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	for(size_t mi = 0; mi < nm; ++mi) out[mi] = (int64_t) found[mi];
	return MPM_OK;
}

int mpm_count_particles_in(mpm_ctx* ctx, int model, const mpm_collision_shape* regions, int nregions, int64_t out[8]) {
	if(!ctx) return MPM_ERR_INVALID;
	const std::string who = "mpm_count_particles_in";
	if(int rc = sink_preconditions(ctx, who, model)) return rc;
	if(!out) return fail(ctx, MPM_ERR_INVALID, who + ": out is missing");
	SinkQuery q;
	if(int rc = sink_regions(ctx, who, regions, nregions, q.sel)) return rc;
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	return sink_count(ctx, model, q, out);
}

int mpm_remove_particles(mpm_ctx* ctx, int model, const mpm_removal* what, mpm_removal_result* out) {
	if(!ctx) return MPM_ERR_INVALID;
	const std::string who = "mpm_remove_particles";
	if(int rc = sink_preconditions(ctx, who, model)) return rc;
	if(!what) return fail(ctx, MPM_ERR_INVALID, who + ": the removal is missing");
	for(int w: what->reserved)
		if(w) return fail(ctx, MPM_ERR_INVALID, who + ": a reserved word of mpm_removal is not 0");
	SinkQuery q;
	if(int rc = sink_regions(ctx, who, what->regions, what->nregions, q.sel)) return rc;
	if(what->nids) {
		if(!what->ids) return fail(ctx, MPM_ERR_INVALID, who + ": ids are missing");
		if(model < 0) return fail(ctx, MPM_ERR_INVALID, who + ": ids name the particles of one model (model >= 0)");
		if(!ctx->track_ids) return fail(ctx, MPM_ERR_INVALID, who + ": ids need a tracked context (mpm_track_particle_ids)");
		const size_t n = ctx->models[model].n;
		for(size_t i = 0; i < what->nids; ++i)
			if(what->ids[i] < 0 || (size_t) what->ids[i] >= n) return fail(ctx, MPM_ERR_INVALID, who + ": id " + std::to_string(what->ids[i]) + " outside 0.." + std::to_string((long long) n - 1));
	}
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	hipStream_t s	   = ctx->s_compute;
	const size_t nm	   = ctx->models.size();
	const size_t table = (size_t) ctx->g.G * ctx->g.G * ctx->g.G;
	mpm_removal_result res {};
	// ---- phase 1: count, split, partition, mark - the context is only read ----
	if(what->nids) {
		const size_t n = ctx->models[model].n;
		RELAY_ALLOC(q.bitmap.alloc((n + 31) / 32, s));
		RELAY_ALLOC(q.d_ids.alloc(what->nids, s));
		HIP_TRY(hipMemcpyAsync(q.d_ids, what->ids, sizeof(int) * what->nids, hipMemcpyHostToDevice, s));
		sink_bitmap_kernel<<<cdiv(what->nids, 256), 256, 0, s>>>(what->nids, q.d_ids, q.bitmap);
		q.sel.bitmap = q.bitmap;
		q.sel.nbits	 = (unsigned) n;
	}
	if(int rc = sink_count(ctx, model, q, res.removed)) return rc;
	size_t selected = 0;
	for(size_t mi = 0; mi < nm; ++mi) selected += (size_t) res.removed[mi];
	if(out) *out = res;
	if(selected == 0) return MPM_OK;// (relaid = 0: nothing was written, the still path stays on offer)
	const bool wants_list = what->removed_xyz || what->removed_ids || what->removed_model;
	if(wants_list && what->capacity < selected)
		return fail(ctx, MPM_ERR_CAPACITY, who + ": " + std::to_string(selected) + " particles are selected, the removed-particle arrays hold " + std::to_string(what->capacity));
	double before[4], after[4];
	if(int rc = mpm_grid_totals(ctx, before)) return rc;
	std::vector<EmitColumns> cols(nm);
	DevBuf<unsigned long long> d_gathered;// [mi] survivors of model mi, [nm] the removed list's length
	DevBuf<int> d_flags;
	DevBuf<float> d_rxyz;
	DevBuf<int> d_rids, d_rmodel;
	RELAY_ALLOC(d_gathered.alloc(nm + 1, s));
	RELAY_ALLOC(d_flags.alloc(2, s));
	RELAY_ALLOC(d_rxyz.alloc(3 * selected, s));
	RELAY_ALLOC(d_rids.alloc(selected, s));
	RELAY_ALLOC(d_rmodel.alloc(selected, s));
	const SinkRemoved gone {d_rxyz.p, d_rids.p, d_rmodel.p, (unsigned long long) selected, d_gathered + nm};
	size_t survivors = 0;
	for(size_t mi = 0; mi < nm; ++mi) {
		const Model& m = ctx->models[mi];
		EmitColumns& c = cols[mi];
		c.live = c.total = (size_t) (m.bucketed - res.removed[mi]);
		c.tracked		 = ctx->track_ids;
		survivors += c.total;
		if(int rc = relay_alloc_columns(ctx, who, c)) return rc;
		if(!m.bucketed || !ctx->pbc) continue;
		if(model >= 0 && (int) mi != model)// (a model the call does not select: emission's gather, as it stands)
			emit_gather_kernel<<<ctx->pbc, kReadoutThreads, 0, s>>>(make_readout_args(ctx, m), c.view(), (unsigned long long) c.live, d_gathered + mi);
		else
			sink_gather_kernel<<<ctx->pbc, kReadoutThreads, 0, s>>>(make_readout_args(ctx, m), q.sel, (int) mi, c.view(), (unsigned long long) c.live, d_gathered + mi, gone);
	}
	{
		std::vector<unsigned long long> gathered(nm + 1);
		HIP_TRY(hipMemcpyAsync(gathered.data(), d_gathered, sizeof(unsigned long long) * (nm + 1), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(s));
		for(size_t mi = 0; mi < nm; ++mi)
			if(gathered[mi] != cols[mi].live)
				return fail(ctx, MPM_ERR_INTERNAL, who + ": the lists of model " + std::to_string(mi) + " hold " + std::to_string(gathered[mi]) + " survivors, the count pass left " + std::to_string(cols[mi].live));
		if(gathered[nm] != selected) return fail(ctx, MPM_ERR_INTERNAL, who + ": " + std::to_string(gathered[nm]) + " particles gathered for removal, " + std::to_string(selected) + " counted");
	}
	ScratchPartition SP;
	if(int rc = relay_scratch_partition(ctx, who, cols, survivors, SP)) return rc;
	const int pbc = SP.pbc, nbc = SP.nbc;
	std::vector<DevBuf<int>> counts(nm);
	std::vector<int> bins(nm, 0);
	if(int rc = relay_count_bins(ctx, who, cols, SP, counts, bins, d_flags)) return rc;
	// the old grid and its keys, kept aside; the removed particles' nodes marked in the old numbering; the scratch mass grid and the new marks
	const int r = ctx->rollid, old_nbc = ctx->nbc;
	DevBuf<float> old_grid, mass_grid;
	DevBuf<int> old_keys;
	DevBuf<unsigned long long> old_marks, new_marks;
	RELAY_ALLOC(old_grid.alloc(256 * (size_t) old_nbc, s));
	RELAY_ALLOC(old_keys.alloc(3 * (size_t) old_nbc, s));
	RELAY_ALLOC(old_marks.alloc((size_t) old_nbc, s));
	RELAY_ALLOC(new_marks.alloc((size_t) nbc, s));
	RELAY_ALLOC(mass_grid.alloc(256 * (size_t) nbc, s));
	HIP_TRY(hipMemcpyAsync(old_grid, ctx->grid[0], sizeof(float) * 256 * (size_t) old_nbc, hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipMemcpyAsync(old_keys, ctx->part[r].keys, sizeof(int) * 3 * (size_t) old_nbc, hipMemcpyDeviceToDevice, s));
	sink_mark_kernel<<<cdiv(selected, 256), 256, 0, s>>>(ctx->g, selected, d_rxyz, ctx->part[r].table, old_nbc, old_marks);
	std::vector<float> h_rxyz;
	std::vector<int> h_rids, h_rmodel;
	if(what->removed_xyz) h_rxyz.resize(3 * selected);
	if(what->removed_ids) h_rids.resize(selected);
	if(what->removed_model) h_rmodel.resize(selected);
	if(what->removed_xyz) HIP_TRY(hipMemcpyAsync(h_rxyz.data(), d_rxyz, sizeof(float) * 3 * selected, hipMemcpyDeviceToHost, s));
	if(what->removed_ids) HIP_TRY(hipMemcpyAsync(h_rids.data(), d_rids, sizeof(int) * selected, hipMemcpyDeviceToHost, s));
	if(what->removed_model) HIP_TRY(hipMemcpyAsync(h_rmodel.data(), d_rmodel, sizeof(int) * selected, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	// ---- phase 2: nothing refuses from here on (capacities neither shrink nor grow: the survivors need no more than the context holds) ----
	phase_call(ctx);
	const GridCfg& g = ctx->g;
	if(int rc = relay_install(ctx, cols, SP, bins)) return rc;
	// the grid: zero, the old blocks under their new numbers with their marks, the survivors' set-up mass beside it (m.list[1] and m.size are as
	// lay_model_bins left them), the marked nodes rescaled
	HIP_TRY(hipMemsetAsync(ctx->grid[0], 0, sizeof(float) * 256 * (size_t) nbc, s));
	HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int) * 2, s));
	if(old_nbc) sink_carry_grid_kernel<<<std::min(2048u, cdiv(old_nbc, 4)), 256, 0, s>>>(g, old_nbc, nbc, old_keys, old_grid, old_marks, ctx->part[r].table, ctx->grid[0], new_marks, d_flags);
	for(size_t mi = 0; mi < nm; ++mi) {
		const Model& m = ctx->models[mi];
		if(!cols[mi].total || !pbc) continue;
		rasterize_blocks_kernel<<<pbc, 256, 0, s>>>(g, cols[mi].xyz, m.list[1], m.size, ctx->part[r].keys, ctx->part[r].table, mass_grid, m.mc.mass, 0.f, 0.f, 0.f);
	}
	if(nbc) sink_rescale_grid_kernel<<<std::min(2048u, cdiv(nbc, 4)), 256, 0, s>>>(nbc, new_marks, mass_grid, ctx->grid[0]);
	int rc = launch_prepare(ctx, PrepareFor::Setup);
	if(rc) return rc;
	HIP_TRY(hipGetLastError());
	rc = read_status(ctx);
	if(rc) return rc;
	{
		int flag = 0;
		HIP_TRY(hipMemcpy(&flag, d_flags, sizeof(int), hipMemcpyDeviceToHost));
		if(flag & kSinkCarryMiss) return fail(ctx, MPM_ERR_INTERNAL, who + ": a dropped block of the old grid holds mass at a node no removed particle reaches");
	}
	// the books: n stays (everything the model was ever given), the removed particles balance through books_bias
	if(int rc2 = relay_books(ctx, who, cols, bins)) return rc2;
	for(size_t mi = 0; mi < nm; ++mi) ctx->models[mi].removed += res.removed[mi];
	ctx->books_bias += (long long) selected;
	ctx->relaid = true;
	if(int rc2 = mpm_grid_totals(ctx, after)) return rc2;
	res.mass = before[0] - after[0];
	for(int d = 0; d < 3; ++d) res.momentum[d] = before[1 + d] - after[1 + d];
	res.relaid = 1;
	if(out) *out = res;
	if(what->removed_xyz) memcpy(what->removed_xyz, h_rxyz.data(), sizeof(float) * 3 * selected);
	if(what->removed_ids) memcpy(what->removed_ids, h_rids.data(), sizeof(int) * selected);
	if(what->removed_model) memcpy(what->removed_model, h_rmodel.data(), sizeof(int) * selected);
	return MPM_OK;
}
#undef RELAY_ALLOC

// Heightfield ----------------------------------------------------------------------------------------------------------------------------
// mpm_collision_object + mpm_heightfield -> the slot and the table's description (table = nullptr: the caller's); nullptr, or the message
// that names the offending field
static const char* make_heightfield_slot(const mpm_collision_object* obj, const mpm_heightfield* hf, ShapeSlot& out, Heightfield& f) {
	if(hf->nx < kHeightfieldMinSamples || hf->nx > MPM_HEIGHTFIELD_MAX_SAMPLES) return "collision heightfield: nx outside 2..4096";
	if(hf->nz < kHeightfieldMinSamples || hf->nz > MPM_HEIGHTFIELD_MAX_SAMPLES) return "collision heightfield: nz outside 2..4096";
	if(!(hf->spacing > 0.f) || !std::isfinite(hf->spacing)) return "collision heightfield: spacing must be finite and > 0";
	if(hf->origin[0] != hf->origin[0] || hf->origin[1] != hf->origin[1]) return "collision heightfield: NaN in origin";
	if(!boundary_type_ok(obj)) return "collision heightfield: boundary type outside 0..2";
	out					 = ShapeSlot {};
	out.obj				 = slot_object(obj);
	out.shape.kind		 = kShapeHeightfield;
	out.shape.inside_out = hf->inside_out ? 1 : 0;
	f					 = Heightfield {};
	f.nx				 = hf->nx;
	f.nz				 = hf->nz;
	f.origin[0]			 = hf->origin[0];
	f.origin[1]			 = hf->origin[1];
	f.spacing			 = hf->spacing;
	f.inside_out		 = out.shape.inside_out;
	return nullptr;
}

int mpm_set_collision_heightfield(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_heightfield* hf, const float* heights) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!slot_ok(slot)) return fail(ctx, MPM_ERR_INVALID, "collision heightfield: slot outside 0..3");
	SlotOccupant o;
	if(!obj) return install_slot(ctx, slot, o, nullptr);
	if(!hf) return fail(ctx, MPM_ERR_INVALID, "collision heightfield: obj without hf");
	if(!heights) return fail(ctx, MPM_ERR_INVALID, "collision heightfield: obj without heights");
	Heightfield& f = o.hf;
	if(const char* msg = make_heightfield_slot(obj, hf, o.shape, f)) return fail(ctx, MPM_ERR_INVALID, msg);
	const size_t n = (size_t) f.nx * f.nz;
	std::vector<float4> table(n);
	if(!heightfield_build(heights, f.nx, f.nz, f.spacing, table.data())) return fail(ctx, MPM_ERR_INVALID, "collision heightfield: a height or a derived table entry is not finite");
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(o.table.alloc(n, ctx->s_compute));
	if(hipError_t e = hipMemcpy(o.table, table.data(), sizeof(float4) * n, hipMemcpyHostToDevice))
		return fail(ctx, MPM_ERR_DEVICE, std::string("collision heightfield: copying the table -> ") + hipGetErrorString(e));
	return install_slot(ctx, slot, o, obj);
}

// Triangle mesh -> level-set field (mpm_collision_mesh.hpp) --------------------------------------------------------------------------------
// What the three consumers of a mesh (this field, a volume's table, the mesh fill) do with it on the host: mesh_build under the API's two
// limits, the extent behind the walk's slack, and the records on the device - released with the scope that owns this.
struct MeshRecords {
	std::vector<MeshTri> rec;
	std::vector<MeshPseudo> pseudo;
	DevBuf<MeshTri> d_rec;
	DevBuf<MeshPseudo> d_pseudo;
	float extent = 0.f;// largest coordinate magnitude in play: the caller's starting value (the domain's 1, or 0 and a box's corners later) or a vertex's
	// empty, or why the mesh is refused ("collision mesh: ...", mesh_build's)
	std::string build(const float* verts, size_t nv, const int32_t* tris, size_t nt, float extent0) {
		MeshReport rep;
		mesh_build(verts, nv, tris, nt, MPM_MESH_MAX_VERTICES, MPM_MESH_MAX_TRIANGLES, rec, pseudo, rep);
		extent = extent0;
		for(size_t i = 0; rep.reason.empty() && i < 3 * nv; ++i) extent = std::max(extent, std::fabs(verts[i]));
		return rep.reason;
	}
	hipError_t alloc(hipStream_t s) {
		const hipError_t e = d_rec.alloc(rec.size(), s);
		return e == hipSuccess ? d_pseudo.alloc(rec.size(), s) : e;
	}
	hipError_t upload() {
		const hipError_t e = hipMemcpy(d_rec.p, rec.data(), sizeof(MeshTri) * rec.size(), hipMemcpyHostToDevice);
		return e == hipSuccess ? hipMemcpy(d_pseudo.p, pseudo.data(), sizeof(MeshPseudo) * rec.size(), hipMemcpyHostToDevice) : e;
	}
	float slack(float spacing) const { return std::max(0.25f * spacing, extent * 0x1p-12f); }
};

// The table of `box` (dims, origin, spacing; its inside_out is the query's, the argument is what goes into the words) from a built mesh:
// wait for the device, allocate the table and the records, upload, run collision_mesh_table_kernel.  MPM_OK: out holds the table.
// Anything else: out is empty (the records go with m) and the context is untouched; the message reads "<who>: ... the <noun> of n <unit> ...".
static int mesh_table_build(mpm_ctx* ctx, MeshRecords& m, const Volume& box, int inside_out, const char* who, const char* noun, const char* unit, DevBuf<float4>& out) {
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	const size_t n = (size_t) box.dims[0] * (size_t) box.dims[1] * (size_t) box.dims[2], nt = m.rec.size();
	DevBuf<float4> table;
	if(table.alloc(n, ctx->s_compute) != hipSuccess || m.alloc(ctx->s_compute) != hipSuccess) {
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, std::string(who) + ": no device memory for the " + noun + " of " + std::to_string(n) + " " + unit + " and " + std::to_string(nt) + " triangle records");
	}
	hipError_t e = m.upload();
	if(e == hipSuccess) {
		const unsigned tiles = (unsigned) ((box.dims[0] + 3) >> 2) * (unsigned) ((box.dims[1] + 3) >> 2) * (unsigned) ((box.dims[2] + 3) >> 2);
		collision_mesh_table_kernel<<<tiles, 64, 0, ctx->s_compute>>>(m.d_rec.p, m.d_pseudo.p, (int) nt, box.dims[0], box.dims[1], box.dims[2], box.origin[0], box.origin[1], box.origin[2], box.spacing,
																	  m.slack(box.spacing), inside_out, table);
		e = hipGetLastError();
	}
	if(e == hipSuccess) e = hipStreamSynchronize(ctx->s_compute);
	if(e != hipSuccess) return fail(ctx, MPM_ERR_DEVICE, std::string(who) + ": building the " + noun + " -> " + hipGetErrorString(e));
	out = std::move(table);
	return MPM_OK;
}

// Order: every host check, then the new field and the records are allocated beside the installed field, filled, and only then does the old
// field go: a refusal - invalid mesh, no memory, a device error - leaves the context as it was.  Replacing a field so needs room for two
// for the duration of the call.
int mpm_set_collision_mesh(mpm_ctx* ctx, const mpm_collision_object* obj, const mpm_collision_mesh* opt, const float* verts, size_t nv, const int32_t* tris, size_t nt) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!obj) return fail(ctx, MPM_ERR_INVALID, "collision mesh: NULL obj (mpm_set_collision_object(ctx, NULL, ...) removes the object)");
	if(!verts || !tris) return fail(ctx, MPM_ERR_INVALID, "collision mesh: NULL verts or tris");
	if(!boundary_type_ok(obj)) return fail(ctx, MPM_ERR_INVALID, "collision mesh: boundary type outside 0..2");
	MeshRecords m;
	const std::string why = m.build(verts, nv, tris, nt, 1.f);
	if(!why.empty()) return fail(ctx, MPM_ERR_INVALID, why);
	const int N = 1 << ctx->cfg.domain_bits;
	Volume nodes {};// the domain's nodes as a table: N^3 samples dx apart from 0
	nodes.dims[0] = nodes.dims[1] = nodes.dims[2] = N;
	nodes.spacing = 1.f / (float) N;
	DevBuf<float4> field;
	if(int rc = mesh_table_build(ctx, m, nodes, opt && opt->inside_out ? 1 : 0, "collision mesh", "field", "nodes", field)) return rc;
	ctx->d_sdf			   = std::move(field);
	ctx->collision		   = slot_object(obj);
	ctx->collision.field   = ctx->d_sdf;
	ctx->has_collision	   = true;
	ctx->collision_running = false;// installing an object stops the clock
	return MPM_OK;
}

// The box lo + [0, dims) of a device table of (., d1, d2) entries to the host (the caller has checked that it lies inside the table)
static int read_table_box(mpm_ctx* ctx, const char* who, const float4* table, int d1, int d2, const int lo[3], const int dims[3], float* out4) {
	const size_t n = (size_t) dims[0] * (size_t) dims[1] * (size_t) dims[2];
	HIP_TRY(hipSetDevice(ctx->device));
	DevBuf<float4> stage;
	if(stage.alloc(n, ctx->s_compute) != hipSuccess) {
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, std::string(who) + ": no device memory for the box");
	}
	collision_table_box_kernel<<<cdiv(n, 256), 256, 0, ctx->s_compute>>>(table, d1, d2, lo[0], lo[1], lo[2], dims[0], dims[1], dims[2], stage.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(ctx->s_compute));
	HIP_TRY(hipMemcpy(out4, stage.p, sizeof(float4) * n, hipMemcpyDeviceToHost));
	return MPM_OK;
}

int mpm_get_collision_field(mpm_ctx* ctx, const int lo[3], const int dims[3], float* out4) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!lo || !dims || !out4) return fail(ctx, MPM_ERR_INVALID, "mpm_get_collision_field: NULL argument");
	if(!ctx->has_collision || !ctx->d_sdf) return fail(ctx, MPM_ERR_INVALID, "mpm_get_collision_field: no level-set collision object installed");
	const int N = 1 << ctx->cfg.domain_bits;
	for(int d = 0; d < 3; ++d) {
		if(dims[d] < 1) return fail(ctx, MPM_ERR_INVALID, "mpm_get_collision_field: a dims entry < 1");
		if(lo[d] < 0 || lo[d] >= N || dims[d] > N - lo[d]) return fail(ctx, MPM_ERR_INVALID, "mpm_get_collision_field: the box leaves [0, N)^3");
	}
	return read_table_box(ctx, "mpm_get_collision_field", ctx->d_sdf, N, N, lo, dims, out4);
}

// Volume: a local level-set box in a slot (mpm_collision_volume.hpp) ----------------------------------------------------------------------------
// mpm_collision_object + mpm_collision_volume -> the slot and the table's description (table = nullptr: the caller's); nullptr, or the message
// that names the offending field.  zero_dims_ok: a mesh install, whose dims {0, 0, 0} ask for the box to be sized from the mesh.
static const char* make_volume_slot(const mpm_collision_object* obj, const mpm_collision_volume* vol, bool zero_dims_ok, ShapeSlot& out, Volume& v) {
	const bool zero = vol->dims[0] == 0 && vol->dims[1] == 0 && vol->dims[2] == 0;
	if(zero && !zero_dims_ok) return "collision volume: dims are all zero without a mesh to size the box from";
	if(!zero) {
		long long total = 1;
		for(int d = 0; d < 3; ++d) {
			if(vol->dims[d] < kVolumeMinSamples || vol->dims[d] > MPM_VOLUME_MAX_SAMPLES) return "collision volume: a dims entry outside 2..1024";
			total *= vol->dims[d];
		}
		if(total > kVolumeMaxTable) return "collision volume: dims whose product exceeds 2^27 samples";
	}
	if(!(vol->spacing > 0.f) || !std::isfinite(vol->spacing)) return "collision volume: spacing must be finite and > 0";
	for(int d = 0; d < 3; ++d)
		if(vol->origin[d] != vol->origin[d]) return "collision volume: NaN in origin";
	if(vol->pad < 0) return "collision volume: pad < 0";
	if(!boundary_type_ok(obj)) return "collision volume: boundary type outside 0..2";
	out					 = ShapeSlot {};
	out.obj				 = slot_object(obj);
	out.shape.kind		 = kShapeVolume;
	out.shape.inside_out = vol->inside_out ? 1 : 0;
	v					 = Volume {};
	for(int d = 0; d < 3; ++d) v.dims[d] = vol->dims[d], v.origin[d] = vol->origin[d];
	v.spacing	 = vol->spacing;
	v.inside_out = out.shape.inside_out;
	return nullptr;
}
// (x - x == 0 exactly for every finite x, NaN for an infinity or a NaN)
static bool volume_samples_finite(const float* field4, size_t cells) {
	for(size_t i = 0; i < 4 * cells; ++i)
		if(!(field4[i] - field4[i] == 0.f)) return false;
	return true;
}
// the descriptor as installed: what mpm_get_collision_volume hands back
static mpm_collision_volume volume_descriptor(const Volume& v, int pad) {
	mpm_collision_volume d {};
	for(int k = 0; k < 3; ++k) d.dims[k] = v.dims[k], d.origin[k] = v.origin[k];
	d.spacing	 = v.spacing;
	d.inside_out = v.inside_out;
	d.pad		 = pad;
	return d;
}

int mpm_set_collision_volume(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* field4) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!slot_ok(slot)) return fail(ctx, MPM_ERR_INVALID, "collision volume: slot outside 0..3");
	SlotOccupant o;
	if(!obj) return install_slot(ctx, slot, o, nullptr);
	if(!vol) return fail(ctx, MPM_ERR_INVALID, "collision volume: obj without vol");
	if(!field4) return fail(ctx, MPM_ERR_INVALID, "collision volume: obj without field4");
	Volume& v = o.vol;
	if(const char* msg = make_volume_slot(obj, vol, false, o.shape, v)) return fail(ctx, MPM_ERR_INVALID, msg);
	const size_t n = (size_t) v.dims[0] * (size_t) v.dims[1] * (size_t) v.dims[2];
	if(!volume_samples_finite(field4, n)) return fail(ctx, MPM_ERR_INVALID, "collision volume: a sample of field4 is not finite");
	HIP_TRY(hipSetDevice(ctx->device));
	if(o.table.alloc(n, ctx->s_compute) != hipSuccess) {
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, "collision volume: no device memory for the table of " + std::to_string(n) + " samples");
	}
	if(hipError_t e = hipMemcpy(o.table, field4, sizeof(float4) * n, hipMemcpyHostToDevice))
		return fail(ctx, MPM_ERR_DEVICE, std::string("collision volume: copying the table -> ") + hipGetErrorString(e));
	o.desc	= volume_descriptor(v, vol->pad);
	return install_slot(ctx, slot, o, obj);
}

// Order, as for mpm_set_collision_mesh: every host check, then the table and the records are allocated beside the slot's old occupant, the
// table is filled, and only then does install_slot free the old occupant's: a refusal - invalid mesh or box, no memory, a device error -
// leaves the slot, the clock and every other slot as they were.
int mpm_set_collision_volume_mesh(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* verts, size_t nv, const int32_t* tris, size_t nt) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!slot_ok(slot)) return fail(ctx, MPM_ERR_INVALID, "collision volume: slot outside 0..3");
	SlotOccupant o;
	if(!obj) return install_slot(ctx, slot, o, nullptr);
	if(!vol) return fail(ctx, MPM_ERR_INVALID, "collision volume: obj without vol");
	if(!verts || !tris) return fail(ctx, MPM_ERR_INVALID, "collision volume: NULL verts or tris");
	Volume& v = o.vol;
	if(const char* msg = make_volume_slot(obj, vol, true, o.shape, v)) return fail(ctx, MPM_ERR_INVALID, msg);
	MeshRecords m;
	const std::string why = m.build(verts, nv, tris, nt, 0.f);
	if(!why.empty()) return fail(ctx, MPM_ERR_INVALID, "collision volume: " + why);
	int pad = vol->pad;
	if(v.dims[0] == 0) {
		pad = pad ? pad : 2;
		if(!volume_autosize(verts, nv, v.spacing, pad, v.origin, v.dims))
			return fail(ctx, MPM_ERR_INVALID, "collision volume: dims sized from the mesh's bounding box, spacing and pad leave 2..1024 per axis or 2^27 samples");
	}
	for(int d = 0; d < 3; ++d) m.extent = std::max(m.extent, std::max(std::fabs(v.origin[d]), std::fabs(v.origin[d] + (float) (v.dims[d] - 1) * v.spacing)));// the box's corners count too
	if(int rc = mesh_table_build(ctx, m, v, 0, "collision volume", "table", "samples", o.table)) return rc;
	o.desc	= volume_descriptor(v, pad);
	return install_slot(ctx, slot, o, obj);
}

int mpm_get_collision_volume(mpm_ctx* ctx, int slot, mpm_collision_volume* vol_out, const int lo[3], const int dims[3], float* out4) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!slot_ok(slot)) return fail(ctx, MPM_ERR_INVALID, "collision volume: slot outside 0..3");
	if(ctx->shape[slot].shape.kind != kShapeVolume || !ctx->vol[slot].table) return fail(ctx, MPM_ERR_INVALID, "collision volume: the slot holds no volume");
	const Volume& v = ctx->vol[slot];
	if(out4) {
		if(!lo || !dims) return fail(ctx, MPM_ERR_INVALID, "collision volume: out4 without lo or dims");
		for(int d = 0; d < 3; ++d) {
			if(dims[d] < 1) return fail(ctx, MPM_ERR_INVALID, "collision volume: a dims entry of the box < 1");
			if(lo[d] < 0 || lo[d] >= v.dims[d] || dims[d] > v.dims[d] - lo[d]) return fail(ctx, MPM_ERR_INVALID, "collision volume: the box leaves the table");
		}
	}
	if(vol_out) *vol_out = ctx->vol_desc[slot];
	return out4 ? read_table_box(ctx, "collision volume", v.table, v.dims[1], v.dims[2], lo, dims, out4) : MPM_OK;
}

// Mesh-sampled models (mpm_mesh_fill.hpp) -------------------------------------------------------------------------------------------------
// One host routine in two halves for both entry points: mesh_fill_count validates, uploads the records, classifies the tiles and scans
// their counts - the total is the only value read back -, mesh_fill_emit writes the points into an array of that size.  Everything the
// plan owns (records, masks, counts, offsets) is released with it, on every exit path.
namespace {
struct MeshFillPlan {
	MeshFillArgs a {};
	unsigned ntiles = 0, ngroups = 0;
	unsigned long long total = 0, shortcuts = 0;
	MeshRecords mesh;
	DevBuf<unsigned char> masks;
	DevBuf<unsigned> counts, bsum;
	DevBuf<unsigned long long> boff;// [ngroups] the groups' offsets, [ngroups] the total, [ngroups + 1] the shortcut tiles (statistics)
	float ms[3] = {0.f, 0.f, 0.f};		// classify, scan, emit - measured only when asked for
};
// Events around the kernels of a timed call; released with the scope
struct MeshFillEvents {
	hipEvent_t e[3] = {nullptr, nullptr, nullptr};
	bool on			= false;
	explicit MeshFillEvents(bool timed) {
		on = timed;
		for(int i = 0; on && i < 3; ++i) on = hipEventCreate(&e[i]) == hipSuccess;
	}
	~MeshFillEvents() {
		for(hipEvent_t x: e)
			if(x) hipEventDestroy(x);
	}
	void mark(int i, hipStream_t s) {
		if(on) hipEventRecord(e[i], s);
	}
	float between(int i, int j) {
		float ms = 0.f;
		if(on) hipEventElapsedTime(&ms, e[i], e[j]);
		return ms;
	}
};
}// namespace

#define FILL_TRY(expr)                                                                        \
	do {                                                                                      \
		hipError_t e_ = (expr);                                                               \
		if(e_ != hipSuccess) {                                                                \
			err = std::string(who) + ": " + #expr + " -> " + hipGetErrorString(e_);           \
			return MPM_ERR_DEVICE;                                                            \
		}                                                                                     \
	} while(0)

static int mesh_fill_count(std::string& err, const char* who, int bits, const float* verts, size_t nv, const int32_t* tris, size_t nt, const mpm_mesh_fill* opt, hipStream_t s,
						   MeshFillPlan& P, bool timed) {
	auto refuse = [&](int code, const std::string& why) {
		err = std::string(who) + ": " + why;
		return code;
	};
	if(!verts || !tris) return refuse(MPM_ERR_INVALID, "NULL verts or tris");
	const float margin = opt ? opt->margin : 0.f;
	if(!(margin >= 0.f) || !std::isfinite(margin)) return refuse(MPM_ERR_INVALID, "margin must be finite and >= 0");
	const std::string why = P.mesh.build(verts, nv, tris, nt, 1.f);// (the extent starts at the domain's 1, as for the field)
	if(!why.empty()) return refuse(MPM_ERR_INVALID, why);
	const int N		   = 1 << bits;
	const bool use_box = opt && opt->use_box;
	MeshFillRange r;
	if(!mesh_fill_range(N, verts, nv, use_box ? opt->lo : nullptr, use_box ? opt->hi : nullptr, r)) return refuse(MPM_ERR_INVALID, "lo / hi outside [0, N]");
	P.a.dx	   = 1.f / (float) N;
	P.a.slack  = P.mesh.slack(P.a.dx);
	P.a.margin = margin;
	for(int d = 0; d < 3; ++d) P.a.lo[d] = r.lo[d], P.a.hi[d] = r.hi[d], P.a.tlo[d] = r.tlo[d], P.a.tn[d] = r.tn[d];
	P.ntiles = (unsigned) r.tn[0] * (unsigned) r.tn[1] * (unsigned) r.tn[2];// at most 256^3
	P.total = P.shortcuts = 0;
	if(!P.ntiles) return MPM_OK;
	P.ngroups = cdiv(P.ntiles, kMeshFillGroup);
	if(P.mesh.alloc(s) != hipSuccess || P.masks.alloc((size_t) P.ntiles * 64, s) != hipSuccess || P.counts.alloc(P.ntiles, s) != hipSuccess
	   || P.bsum.alloc(P.ngroups, s) != hipSuccess || P.boff.alloc((size_t) P.ngroups + 2, s) != hipSuccess) {
		(void) hipGetLastError();
		return refuse(MPM_ERR_CAPACITY, "no device memory for the work buffers of " + std::to_string(P.ntiles) + " tiles and " + std::to_string(nt) + " triangle records");
	}
	FILL_TRY(P.mesh.upload());
	MeshFillEvents ev(timed);
	ev.mark(0, s);
	mesh_fill_classify_kernel<<<P.ntiles, 64, 0, s>>>(P.mesh.d_rec.p, P.mesh.d_pseudo.p, (int) nt, P.a, P.masks.p, P.counts.p, P.boff.p + P.ngroups + 1);
	FILL_TRY(hipGetLastError());
	ev.mark(1, s);
	mesh_fill_scan_block_kernel<<<P.ngroups, 256, 0, s>>>(P.counts.p, P.ntiles, P.bsum.p);
	FILL_TRY(hipGetLastError());
	mesh_fill_scan_top_kernel<<<1, 1024, 0, s>>>(P.bsum.p, P.ngroups, P.boff.p);
	FILL_TRY(hipGetLastError());
	ev.mark(2, s);
	unsigned long long tail[2] = {0, 0};
	FILL_TRY(hipMemcpyAsync(tail, P.boff.p + P.ngroups, sizeof(tail), hipMemcpyDeviceToHost, s));
	FILL_TRY(hipStreamSynchronize(s));
	P.total		= tail[0];
	P.shortcuts = tail[1];
	P.ms[0]		= ev.between(0, 1);
	P.ms[1]		= ev.between(1, 2);
	return MPM_OK;
}

// d_xyz: 3 P.total floats on the device
static int mesh_fill_emit(std::string& err, const char* who, MeshFillPlan& P, float* d_xyz, hipStream_t s, bool timed) {
	if(!P.total) return MPM_OK;
	MeshFillEvents ev(timed);
	ev.mark(0, s);
	mesh_fill_emit_kernel<<<P.ntiles, 64, 0, s>>>(P.masks.p, P.counts.p, P.boff.p, P.a, d_xyz, P.total);
	FILL_TRY(hipGetLastError());
	ev.mark(1, s);
	FILL_TRY(hipStreamSynchronize(s));
	P.ms[2] = ev.between(0, 1);
	return MPM_OK;
}
#undef FILL_TRY

// out8 (may be NULL): {points, tiles, shortcut tiles, classify ms, scan ms, emit ms, 0, 0} of a timed call
static int sample_mesh(int domain_bits, const float* verts, size_t nv, const int32_t* tris, size_t nt, const mpm_mesh_fill* opt, float* xyz, size_t* n, int device, double* out8) {
	if(!n || domain_bits < 4 || domain_bits > 10) return MPM_ERR_INVALID;
	if(hipSetDevice(device) != hipSuccess) return MPM_ERR_DEVICE;
	std::string err;
	MeshFillPlan P;
	if(int rc = mesh_fill_count(err, "mpm_sample_mesh", domain_bits, verts, nv, tris, nt, opt, nullptr, P, out8 != nullptr)) return rc;
	const size_t cap = xyz ? *n : 0;
	if(P.total > SIZE_MAX / (3 * sizeof(float))) return MPM_ERR_CAPACITY;
	*n = (size_t) P.total;
	if(xyz && P.total > cap) return MPM_ERR_CAPACITY;
	if((xyz || out8) && P.total) {
		DevBuf<float> d_xyz;
		if(d_xyz.alloc(3 * (size_t) P.total, nullptr) != hipSuccess) {
			(void) hipGetLastError();
			return MPM_ERR_CAPACITY;
		}
		if(int rc = mesh_fill_emit(err, "mpm_sample_mesh", P, d_xyz.p, nullptr, out8 != nullptr)) return rc;
		if(xyz && hipMemcpy(xyz, d_xyz.p, sizeof(float) * 3 * (size_t) P.total, hipMemcpyDeviceToHost) != hipSuccess) return MPM_ERR_DEVICE;
	}
	if(out8) {
		const double v[8] = {(double) P.total, (double) P.ntiles, (double) P.shortcuts, P.ms[0], P.ms[1], P.ms[2], 0., 0.};
		std::copy(v, v + 8, out8);
	}
	return MPM_OK;
}

int mpm_sample_mesh(int domain_bits, const float* verts, size_t nv, const int32_t* tris, size_t nt, const mpm_mesh_fill* opt, float* xyz, size_t* n, int device) {
	return sample_mesh(domain_bits, verts, nv, tris, nt, opt, xyz, n, device, nullptr);
}

int mpm_test_mesh_fill(int domain_bits, const float* verts, size_t nv, const int32_t* tris, size_t nt, const mpm_mesh_fill* opt, double* out8, int device) {
	if(!out8) return MPM_ERR_INVALID;
	size_t n = 0;
	return sample_mesh(domain_bits, verts, nv, tris, nt, opt, nullptr, &n, device, out8);
}

int mpm_add_model_mesh(mpm_ctx* ctx, int material, const mpm_material_params* params, const float* verts, size_t nv, const int32_t* tris, size_t nt, const mpm_mesh_fill* opt,
					   const float v0[3], int* model_id, size_t* n_out) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!params) return fail(ctx, MPM_ERR_INVALID, "mpm_add_model_mesh: material parameters are missing");
	if(ctx->ready) return fail(ctx, MPM_ERR_INVALID, "mpm_add_model_mesh: models must be added before mpm_initial_setup");
	if(material < 0 || material > 3) return fail(ctx, MPM_ERR_INVALID, "unknown material");
	if((int) ctx->models.size() >= kMaxModels) return fail(ctx, MPM_ERR_CAPACITY, "too many models");
	HIP_TRY(hipSetDevice(ctx->device));
	std::string err;
	MeshFillPlan P;
	if(int rc = mesh_fill_count(err, "mpm_add_model_mesh", ctx->cfg.domain_bits, verts, nv, tris, nt, opt, ctx->s_compute, P, false)) return fail(ctx, rc, err);
	if(P.total > SIZE_MAX / (3 * sizeof(float))) return fail(ctx, MPM_ERR_CAPACITY, "mpm_add_model_mesh: no device memory for " + std::to_string(P.total) + " positions");
	Model m;
	m.material = material;
	m.p		   = *params;
	m.mc	   = make_material_const(*params);
	m.nch	   = material == MPM_J_FLUID ? 4 : (material == MPM_FIXED_COROTATED ? 9 : 10);// as mpm_add_model
	m.n		   = (size_t) P.total;
	for(int d = 0; d < 3; ++d) m.v0[d] = v0 ? v0[d] : 0.f;
	if(m.d_xyz.alloc(3 * m.n, ctx->s_compute) != hipSuccess) {// the model's own array: the emit kernel writes into it
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_add_model_mesh: no device memory for " + std::to_string(P.total) + " positions");
	}
	if(int rc = mesh_fill_emit(err, "mpm_add_model_mesh", P, m.d_xyz, ctx->s_compute, false)) return fail(ctx, rc, err);
	if(model_id) *model_id = (int) ctx->models.size();
	if(n_out) *n_out = m.n;
	ctx->models.push_back(std::move(m));
	return MPM_OK;
}

int mpm_set_collision_clock(mpm_ctx* ctx, int running, float time) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!ctx->has_collision && !ctx->shape_count) return fail(ctx, MPM_ERR_INVALID, "no collision object installed");
	ctx->collision.time	   = time;
	ctx->collision_running = running != 0;
	return MPM_OK;
}
int mpm_get_collision_time(mpm_ctx* ctx, float* time, int* running) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!ctx->has_collision && !ctx->shape_count) return fail(ctx, MPM_ERR_INVALID, "no collision object installed");
	if(time) *time = ctx->collision.time;
	if(running) *running = ctx->collision_running ? 1 : 0;
	return MPM_OK;
}

int mpm_get_capacity(mpm_ctx* ctx, int64_t* block_capacity, int64_t* bin_capacity, int* growth_events) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(block_capacity) *block_capacity = ctx->g.cap;
	if(bin_capacity)
		for(size_t i = 0; i < ctx->models.size() && i < 8; ++i) bin_capacity[i] = (int64_t) ctx->models[i].bin_cap;
	if(growth_events) *growth_events = ctx->capacity_events;
	return MPM_OK;
}

int mpm_get_diagnostics(mpm_ctx* ctx, mpm_diagnostics* d) {
	if(!ctx || !ctx->ready || !d) return MPM_ERR_NOT_READY;
	memset(d, 0, sizeof(*d));
	d->lost_particles = ctx->h_status[ST_LOST];
	d->discarded_p2g  = ctx->h_status[ST_ARENA];
	d->overflow_flags = ctx->h_status[ST_OVERFLOW];
	d->dropped_particles = ctx->h_status[ST_DROPPED];
	d->still_rebuilds	 = ctx->h_status[ST_STILL];
#ifdef MPM_G2P2G_STATS
	for(int i = 0; i < 3; ++i) d->reserved[i] = ctx->h_status[24 + i];// cumulative: iterations, loser lanes, edge lanes (the fourth, iterations with a retry: the bits of mpm_timers.reserved[0])
#endif
	return MPM_OK;
}

int mpm_get_timers(mpm_ctx* ctx, mpm_timers* t) {
	if(!ctx || !t) return MPM_ERR_INVALID;
	*t = ctx->timers;
#ifdef MPM_G2P2G_STATS
	if(ctx->h_status) memcpy(&t->reserved[0], &ctx->h_status[27], sizeof(int));// cumulative iterations with a retry: the int's BITS (tools/g2p2g_stats_run.py)
#endif
	return MPM_OK;
}

// The launch of readout_kernel<kind> for model m: the one place that knows which kinds read the grid.
static void launch_readout(mpm_ctx* ctx, const Model& m, ReadoutKind kind, const ReadoutOut& out, hipStream_t s) {
	if(!ctx->pbc) return;
	const ReadoutArgs a = make_readout_args(ctx, m);
	switch(kind) {
	case kReadState: readout_kernel<kReadState><<<ctx->pbc, kReadoutThreads, 0, s>>>(a, nullptr, out); break;
	case kReadVelocity: readout_kernel<kReadVelocity><<<ctx->pbc, kReadoutThreads, 0, s>>>(a, ctx->grid[0], out); break;
	case kReadMomentum: readout_kernel<kReadMomentum><<<ctx->pbc, kReadoutThreads, 0, s>>>(a, ctx->grid[0], out); break;
	case kReadStress: readout_kernel<kReadStress><<<ctx->pbc, kReadoutThreads, 0, s>>>(a, nullptr, out); break;
	case kReadStressTotals: readout_kernel<kReadStressTotals><<<ctx->pbc, kReadoutThreads, 0, s>>>(a, nullptr, out); break;
	case kReadIds: readout_kernel<kReadIds><<<ctx->pbc, kReadoutThreads, 0, s>>>(a, nullptr, out); break;
	}
}

// One per-particle readout of a model (readout_kernel<kind>: kReadState, kReadVelocity, kReadStress or kReadIds - whose column 1 is the int32 id) into the caller's arrays: host[0] the positions,
// host[1] and host[2] (null: not asked for) kReadoutWidth[kind][c] floats a particle.  Positions are staged in m.d_xyz, the other columns
// in scratch released on every exit path (an output call, once per frame at most).  *n: the capacity of the arrays in, the particles
// written out - MPM_ERR_CAPACITY if that is not all of them.
static int readout_particles(mpm_ctx* ctx, int model, ReadoutKind kind, float* const host[3], size_t* n) {
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s	 = ctx->s_compute;
	Model& m		 = ctx->models[model];
	const size_t cap = std::min(*n, m.n);
	DevBuf<float> scratch[3];
	ReadoutOut out {{m.d_xyz, nullptr, nullptr}, cap, ctx->d_counter, 0.0, nullptr, m.material, m.mc};
	for(int c = 1; c < 3; ++c)
		if(host[c]) {
			HIP_TRY(scratch[c].alloc(kReadoutWidth[kind][c] * cap, s));
			out.col[c] = scratch[c].p;
		}
	if(kind == kReadIds) out.ids = reinterpret_cast<int*>(out.col[1]);
	HIP_TRY(hipMemsetAsync(ctx->d_counter, 0, sizeof(unsigned long long), s));
	launch_readout(ctx, m, kind, out, s);
	HIP_TRY(hipGetLastError());
	unsigned long long count = 0;
	HIP_TRY(hipMemcpyAsync(&count, ctx->d_counter, sizeof(count), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const size_t got = std::min<size_t>(count, cap);
	for(int c = 0; c < 3; ++c)
		if(host[c]) HIP_TRY(hipMemcpy(host[c], out.col[c], sizeof(float) * kReadoutWidth[kind][c] * got, hipMemcpyDeviceToHost));
	*n = got;
	if(count > cap) return fail(ctx, MPM_ERR_CAPACITY, "output array too small");
	return MPM_OK;
}

// output_model, gmpm_simulator.cuh:594-634 (+ state for the parity tests): whatever grid[0] holds
int mpm_retrieve_state(mpm_ctx* ctx, int model, float* xyz, float* state9, float* logjp, size_t* n) {
	if(!ctx || !ctx->ready || model < 0 || model >= (int) ctx->models.size() || !n || !xyz) return MPM_ERR_INVALID;
	float* const host[3] = {xyz, state9, logjp};
	return readout_particles(ctx, model, kReadState, host, n);
}

// Per-particle velocity and affine matrix gathered from grid[0] (mpm_readout.hpp; an extension, the reference has no velocity output).
// The readout of this context's own grid, without the state checks of its callers (mpm_retrieve_velocity, mpm_group_retrieve_velocity).
static int readout_velocity(mpm_ctx* ctx, int model, float* xyz, float* vel, float* affine9, size_t* n) {
	float* const host[3] = {xyz, vel, affine9};
	return readout_particles(ctx, model, kReadVelocity, host, n);
}

// The totals of one model (model >= 0) or of all models (-1), one launch per model into one accumulator of nwords 64-bit words:
// kReadMomentum {count, sum m v_p (3), sum 1/2 m |v_p|^2} from this context's own grid[0]; kReadStressTotals {count, sum V0 tau (6)} and,
// in the eighth word, the float32 bit pattern of the largest von Mises stress (mpm_readout.hpp), handed back as a double.
static int readout_totals(mpm_ctx* ctx, int model, ReadoutKind kind, int nwords, double* out) {
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	DevBuf<double> d_out;
	HIP_TRY(d_out.alloc(nwords, s));
	for(int mi = model < 0 ? 0 : model; mi < (model < 0 ? (int) ctx->models.size() : model + 1); ++mi) {
		Model& m = ctx->models[mi];
		if(m.n) launch_readout(ctx, m, kind, ReadoutOut {{}, 0, nullptr, (double) (kind == kReadMomentum ? m.mc.mass : m.mc.volume), d_out.p, m.material, m.mc}, s);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(double) * nwords, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if(kind == kReadStressTotals) {
		float q;
		std::memcpy(&q, out + kStressSums, sizeof(q));
		out[kStressSums] = (double) q;
	}
	return MPM_OK;
}
static int readout_momentum(mpm_ctx* ctx, int model, double out[5]) {
	return readout_totals(ctx, model, kReadMomentum, kMomentumSums, out);
}

// The state checks of the single-context readouts: NOT_READY, then INVALID for a context of a group and for a grid that holds velocities.
static int readout_state(mpm_ctx* ctx, const char* who) {
	if(ctx->group_refs > 0 || ctx->mgsp_rank >= 0 || ctx->halo_tagged)
		return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": the context belongs (or belonged) to a multi-GPU group; read it out through the group (mpm_group_retrieve_velocity, mpm_group_particle_momentum), which knows whether its grid holds the summed momentum");
	if(!ctx->grid_momentum)
		return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": the grid holds velocities (mpm_grid_update ran after the last rebuild): call mpm_rebuild_partition (or finish the substep) first");
	return MPM_OK;
}

int mpm_retrieve_velocity(mpm_ctx* ctx, int model, float* xyz, float* vel, float* affine9, size_t* n) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(model < 0 || model >= (int) ctx->models.size() || !n || !xyz || !vel) return fail(ctx, MPM_ERR_INVALID, "mpm_retrieve_velocity: bad model or NULL output array");
	if(int rc = readout_state(ctx, "mpm_retrieve_velocity")) return rc;
	return readout_velocity(ctx, model, xyz, vel, affine9, n);
}

int mpm_particle_momentum(mpm_ctx* ctx, int model, double out[5]) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(model < -1 || model >= (int) ctx->models.size() || !out) return fail(ctx, MPM_ERR_INVALID, "mpm_particle_momentum: bad model or NULL output array");
	if(int rc = readout_state(ctx, "mpm_particle_momentum")) return rc;
	return readout_momentum(ctx, model, out);
}

// Per-particle Cauchy stress, J, pressure and von Mises stress (readout_kernel<kReadStress>; an extension, the reference has no stress
// output): from the records alone, so with mpm_retrieve_state's preconditions - any ready context, of a group or not, whatever the grid holds.
int mpm_retrieve_stress(mpm_ctx* ctx, int model, float* xyz, float* stress6, float* scalars3, size_t* n) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(model < 0 || model >= (int) ctx->models.size() || !n || !xyz) return fail(ctx, MPM_ERR_INVALID, "mpm_retrieve_stress: bad model or NULL output array");
	float* const host[3] = {xyz, stress6, scalars3};
	return readout_particles(ctx, model, kReadStress, host, n);
}

int mpm_stress_totals(mpm_ctx* ctx, int model, double out[8]) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(model < -1 || model >= (int) ctx->models.size() || !out) return fail(ctx, MPM_ERR_INVALID, "mpm_stress_totals: bad model or NULL output array");
	return readout_totals(ctx, model, kReadStressTotals, kStressSums + 1, out);
}

// Persistent particle identities (mpm_particle_ids.hpp; an extension, the reference has none) ------------------------------------------
int mpm_track_particle_ids(mpm_ctx* ctx, int on) {
	if(!ctx) return MPM_ERR_INVALID;
	if(ctx->ready) return fail(ctx, MPM_ERR_INVALID, "mpm_track_particle_ids: tracking is chosen before mpm_initial_setup");
	ctx->track_ids = on != 0;
	return MPM_OK;
}
// what both the readout and the blob's writer ask first
static int ids_usable(mpm_ctx* ctx, const char* who) {
	if(!ctx->track_ids) return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": the context does not track particle ids (mpm_track_particle_ids before mpm_initial_setup)");
	if(!ctx->ids_valid) return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": the ids are not valid: a checkpoint was loaded, load its ids with mpm_particle_ids_load");
	return MPM_OK;
}
int mpm_retrieve_ids(mpm_ctx* ctx, int model, float* xyz, int32_t* ids, size_t* n) {
	if(!ctx || !ctx->ready || model < 0 || model >= (int) ctx->models.size() || !n || !xyz) return MPM_ERR_INVALID;
	if(!ids) return fail(ctx, MPM_ERR_INVALID, "mpm_retrieve_ids: NULL ids");
	if(int rc = ids_usable(ctx, "mpm_retrieve_ids")) return rc;
	static_assert(sizeof(int32_t) == sizeof(float), "the id column is staged like a float column");
	float* const host[3] = {xyz, reinterpret_cast<float*>(ids), nullptr};
	return readout_particles(ctx, model, kReadIds, host, n);
}

namespace {
// The companion of a checkpoint: this header, then per model bincount_src * 64 int32 - one per slot of the source bins, in the slot order
// of the checkpoint's bins section.
struct IdsHeader {
	uint64_t magic;// "MPMPIDS1"
	int32_t nmodels, reserved;
	struct {
		int64_t n, bincount_src;
	} models[8];
};
constexpr uint64_t kIdsMagic = 0x31534449504d504dull;
static IdsHeader ids_header(const mpm_ctx* ctx) {
	IdsHeader h {};
	h.magic	  = kIdsMagic;
	h.nmodels = (int32_t) ctx->models.size();
	for(int m = 0; m < h.nmodels; ++m) h.models[m].n = (int64_t) ctx->models[m].n, h.models[m].bincount_src = ctx->models[m].bincount_src;
	return h;
}
static size_t ids_bytes(const IdsHeader& h) {
	size_t b = sizeof(IdsHeader);
	for(int m = 0; m < h.nmodels; ++m) b += sizeof(int32_t) * (size_t) h.models[m].bincount_src * kBin;
	return b;
}
}// namespace

int mpm_particle_ids_size(mpm_ctx* ctx, size_t* bytes) {
	if(!ctx || !ctx->ready || !bytes) return MPM_ERR_NOT_READY;
	if(!ctx->track_ids) return fail(ctx, MPM_ERR_INVALID, "mpm_particle_ids_size: the context does not track particle ids");
	*bytes = ids_bytes(ids_header(ctx));
	return MPM_OK;
}
int mpm_particle_ids_save(mpm_ctx* ctx, void* buf, size_t capacity, size_t* written) {
	if(!ctx || !ctx->ready || !buf) return MPM_ERR_NOT_READY;
	if(int rc = ids_usable(ctx, "mpm_particle_ids_save")) return rc;
	const IdsHeader h = ids_header(ctx);
	const size_t need = ids_bytes(h);
	if(capacity < need) return fail(ctx, MPM_ERR_CAPACITY, "particle id buffer too small: " + std::to_string(need) + " bytes needed");
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	char* out = (char*) buf;
	memcpy(out, &h, sizeof(h));
	size_t o = sizeof(h);
	for(const Model& M: ctx->models) {
		const size_t b = sizeof(int32_t) * (size_t) M.bincount_src * kBin;
		if(b) HIP_TRY(hipMemcpy(out + o, M.ids[ctx->rollid], b, hipMemcpyDeviceToHost));
		o += b;
	}
	if(written) *written = need;
	return MPM_OK;
}
int mpm_particle_ids_load(mpm_ctx* ctx, const void* buf, size_t bytes) {
	if(!ctx || !ctx->ready || !buf) return MPM_ERR_NOT_READY;
	if(!ctx->track_ids) return fail(ctx, MPM_ERR_INVALID, "mpm_particle_ids_load: the context does not track particle ids");
	if(bytes < sizeof(IdsHeader)) return fail(ctx, MPM_ERR_INVALID, "particle ids: truncated header");
	IdsHeader h;
	memcpy(&h, buf, sizeof(h));
	const IdsHeader mine = ids_header(ctx);
	if(h.magic != kIdsMagic) return fail(ctx, MPM_ERR_INVALID, "particle ids: bad magic");
	if(h.nmodels != mine.nmodels) return fail(ctx, MPM_ERR_INVALID, "particle ids: model count differs from the context");
	for(int m = 0; m < h.nmodels; ++m)
		if(h.models[m].n != mine.models[m].n || h.models[m].bincount_src != mine.models[m].bincount_src)
			return fail(ctx, MPM_ERR_INVALID, "particle ids: model " + std::to_string(m) + " differs from the context's current state (particle count or source bins)");
	if(bytes < ids_bytes(mine)) return fail(ctx, MPM_ERR_INVALID, "particle ids: truncated");
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipDeviceSynchronize());
	const char* in = (const char*) buf;
	size_t o	   = sizeof(h);
	for(Model& M: ctx->models) {
		const size_t b = sizeof(int32_t) * (size_t) M.bincount_src * kBin;
		if(b) HIP_TRY(hipMemcpy(M.ids[ctx->rollid], in + o, b, hipMemcpyHostToDevice));
		o += b;
	}
	ctx->ids_valid = true;
	return MPM_OK;
}

int mpm_retrieve_positions(mpm_ctx* ctx, int model, float* xyz, size_t* n) {
	return mpm_retrieve_state(ctx, model, xyz, nullptr, nullptr, n);
}

int mpm_grid_totals(mpm_ctx* ctx, double out[4]) {
	if(!ctx || !ctx->ready || !out) return MPM_ERR_NOT_READY;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	HIP_TRY(hipMemsetAsync(ctx->d_totals, 0, sizeof(double) * 4, s));
	if(ctx->nbc) grid_totals_kernel<<<256, 256, 0, s>>>(ctx->nbc, ctx->grid[0], ctx->d_totals);
	HIP_TRY(hipMemcpyAsync(out, ctx->d_totals, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	return MPM_OK;
}

int mpm_check_table(mpm_ctx* ctx) {
	if(!ctx || !ctx->ready) return -1;
	if(hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->s_compute) != hipSuccess) return -1;
	const Partition& P = ctx->part[ctx->rollid];
	const size_t table = (size_t) ctx->g.G * ctx->g.G * ctx->g.G;
	std::vector<int> t(table), k(3 * (size_t) ctx->ebc);
	if(hipMemcpy(t.data(), P.table, sizeof(int) * table, hipMemcpyDeviceToHost) != hipSuccess) return -1;
	if(ctx->ebc && hipMemcpy(k.data(), P.keys, sizeof(int) * k.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
	long long bad = 0, set = 0;
	for(int v: t) set += v != -1;
	for(int i = 0; i < ctx->ebc; ++i) {
		const int x = k[3 * i], y = k[3 * i + 1], z = k[3 * i + 2];
		const bool in = x >= 0 && y >= 0 && z >= 0 && x < ctx->g.G && y < ctx->g.G && z < ctx->g.G;
		if(!in || t[((size_t) x << (2 * ctx->g.gbits)) | ((size_t) y << ctx->g.gbits) | (size_t) z] != i) ++bad;
	}
	bad += std::llabs(set - (long long) ctx->ebc);
	return (int) std::min<long long>(bad, 0x7fffffff);
}

int mpm_dump_grid(mpm_ctx* ctx, int* keys, float* blocks, size_t* nblocks) {
	if(!ctx || !ctx->ready || !nblocks) return MPM_ERR_NOT_READY;
	if(*nblocks < (size_t) ctx->nbc) return fail(ctx, MPM_ERR_CAPACITY, "grid dump too small");
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipStreamSynchronize(ctx->s_compute));
	if(keys) HIP_TRY(hipMemcpy(keys, ctx->part[ctx->rollid].keys, sizeof(int) * 3 * (size_t) ctx->nbc, hipMemcpyDeviceToHost));
	if(blocks) HIP_TRY(hipMemcpy(blocks, ctx->grid[0], sizeof(float) * 256 * (size_t) ctx->nbc, hipMemcpyDeviceToHost));
	*nblocks = ctx->nbc;
	return MPM_OK;
}

int mpm_dump_block_rows(mpm_ctx* ctx, int model, int32_t* rows, size_t* nblocks) {
	if(!ctx || !ctx->ready || !nblocks) return MPM_ERR_NOT_READY;
	if(model < 0 || model >= (int) ctx->models.size()) return fail(ctx, MPM_ERR_INVALID, "mpm_dump_block_rows: no such model");
	if(*nblocks < (size_t) ctx->pbc) return fail(ctx, MPM_ERR_CAPACITY, "block row dump too small");
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipStreamSynchronize(ctx->s_compute));
	if(rows && ctx->pbc) HIP_TRY(hipMemcpy(rows, ctx->models[model].blockinfo, sizeof(int) * (size_t) kInfoRow * (size_t) ctx->pbc, hipMemcpyDeviceToHost));
	*nblocks = ctx->pbc;
	return MPM_OK;
}

// Eulerian readouts (mpm_grid_field.hpp; an extension, the reference has none): point samples, dense volumes and box totals of grid[0], the
// mass and momentum of the last P2G.  Preconditions those of mpm_retrieve_velocity (readout_state).  Read-only; temporaries are scratch
// released on every exit path, so a context that never calls these allocates and launches nothing for them.
int mpm_sample_grid(mpm_ctx* ctx, const float* xyz, size_t n, float* out4) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(n && (!xyz || !out4)) return fail(ctx, MPM_ERR_INVALID, "mpm_sample_grid: NULL array");
	if(n > ((size_t) 1 << 31)) return fail(ctx, MPM_ERR_INVALID, "mpm_sample_grid: more than 2^31 points in one call");
	if(int rc = readout_state(ctx, "mpm_sample_grid")) return rc;
	if(!n) return MPM_OK;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	DevBuf<float> d_xyz, d_out;
	if(d_xyz.alloc(3 * n, s) != hipSuccess || d_out.alloc(4 * n, s) != hipSuccess) {
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_sample_grid: no device memory for " + std::to_string(n) + " points");
	}
	HIP_TRY(hipMemcpyAsync(d_xyz.p, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, s));
	grid_sample_kernel<<<cdiv(n, kGridFieldThreads), kGridFieldThreads, 0, s>>>(ctx->g, ctx->nbc, ctx->part[ctx->rollid].table, ctx->grid[0], d_xyz.p, n, d_out.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out4, d_out.p, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	return MPM_OK;
}

int mpm_grid_volume(mpm_ctx* ctx, const int origin[3], const int dims[3], int stride, float* out) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(!origin || !dims || !out) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_volume: NULL argument");
	if(stride != 1 && stride != 2 && stride != 4) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_volume: stride " + std::to_string(stride) + " (1, 2 or 4)");
	if(dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_volume: every entry of dims must be at least 1");
	size_t cells = (size_t) dims[0];
	for(int d = 1; d < 3; ++d) {
		if(cells > SIZE_MAX / (size_t) dims[d]) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_volume: the box overflows size_t");
		cells *= (size_t) dims[d];
	}
	if(cells > SIZE_MAX / 16) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_volume: the box overflows size_t");
	if(int rc = readout_state(ctx, "mpm_grid_volume")) return rc;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	DevBuf<float> d_out;
	if(d_out.alloc(4 * cells, s) != hipSuccess) {
		(void) hipGetLastError();// (the context stays usable)
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_grid_volume: no device memory for " + std::to_string(16 * cells) + " bytes");
	}
	VolumeArgs a {};
	const int tile[3] = {kVolTileX / stride, kVolTileY / stride, kVolTileZ / stride};
	unsigned long long ntiles = 1;
	for(int d = 0; d < 3; ++d) {
		a.origin[d] = origin[d];
		a.dims[d]	= dims[d];
		a.tiles[d]	= ((long long) dims[d] + tile[d] - 1) / tile[d];
		ntiles *= (unsigned long long) a.tiles[d];// (<= cells)
	}
	const unsigned nwg = (unsigned) std::min<unsigned long long>(ntiles, 1u << 20);// the kernel strides over the tiles
	const int* table   = ctx->part[ctx->rollid].table;
	if(stride == 1)
		grid_volume_kernel<1><<<nwg, kGridFieldThreads, 0, s>>>(ctx->g, ctx->nbc, table, ctx->grid[0], a, d_out.p);
	else if(stride == 2)
		grid_volume_kernel<2><<<nwg, kGridFieldThreads, 0, s>>>(ctx->g, ctx->nbc, table, ctx->grid[0], a, d_out.p);
	else
		grid_volume_kernel<4><<<nwg, kGridFieldThreads, 0, s>>>(ctx->g, ctx->nbc, table, ctx->grid[0], a, d_out.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, d_out.p, 16 * cells, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	return MPM_OK;
}

int mpm_grid_box_totals(mpm_ctx* ctx, const int lo[3], const int hi[3], double out[5]) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(!lo || !hi || !out) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_box_totals: NULL argument");
	if(int rc = readout_state(ctx, "mpm_grid_box_totals")) return rc;
	BoxArgs box {};
	bool empty = ctx->nbc == 0;
	for(int d = 0; d < 3; ++d) {
		box.lo[d] = std::max(lo[d], 0);
		box.hi[d] = std::min(hi[d], 4 * ctx->g.G);
		empty	  = empty || box.lo[d] >= box.hi[d];
	}
	for(int d = 0; d < kBoxSums; ++d) out[d] = 0.0;
	if(empty) return MPM_OK;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	DevBuf<double> d_out;
	if(d_out.alloc(kBoxSums, s) != hipSuccess) {
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_grid_box_totals: no device memory");
	}
	grid_box_totals_kernel<<<std::min(256u, cdiv(ctx->nbc, kGridFieldThreads / 64)), kGridFieldThreads, 0, s>>>(ctx->nbc, ctx->part[ctx->rollid].keys, ctx->grid[0], box, d_out.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(double) * kBoxSums, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	return MPM_OK;
}

// The iso-surface f = iso_mass of the mass channel (mpm_grid_isosurface.hpp): mpm_grid_volume's preconditions, mpm_halo_keys' capacity
// protocol.  The triangles are staged in device scratch sized by the caller's capacity and released on every exit path; the count runs in
// d_counter.  A count-only call (tri_xyz NULL, or a capacity of 0) allocates nothing.
int mpm_grid_isosurface(mpm_ctx* ctx, float iso_mass, const int lo[3], const int hi[3], float* tri_xyz, float* tri_vel, size_t* n) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(!n) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_isosurface: NULL n");
	if(!(iso_mass > 0.f) || !std::isfinite(iso_mass)) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_isosurface: iso_mass must be finite and > 0");
	if((lo == nullptr) != (hi == nullptr)) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_isosurface: lo and hi are given together or not at all");
	if(!tri_xyz && tri_vel) return fail(ctx, MPM_ERR_INVALID, "mpm_grid_isosurface: tri_vel without tri_xyz");
	if(int rc = readout_state(ctx, "mpm_grid_isosurface")) return rc;
	const size_t cap = tri_xyz ? *n : 0;
	if(cap > SIZE_MAX / (36 * sizeof(float))) return fail(ctx, MPM_ERR_CAPACITY, "mpm_grid_isosurface: no device memory for " + std::to_string(cap) + " triangles");
	if(!ctx->nbc) {
		*n = 0;
		return MPM_OK;
	}
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	DevBuf<float> d_xyz, d_vel;
	if(cap && (d_xyz.alloc(9 * cap, s) != hipSuccess || (tri_vel && d_vel.alloc(9 * cap, s) != hipSuccess))) {
		(void) hipGetLastError();// (the context stays usable; *n is left as it was)
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_grid_isosurface: no device memory for " + std::to_string(cap) + " triangles");
	}
	IsoArgs a {};
	for(int d = 0; d < 3; ++d) {
		a.lo[d] = lo ? lo[d] : -1;
		a.hi[d] = hi ? hi[d] : 4 * ctx->g.G;
	}
	a.iso	   = iso_mass;
	a.capacity = cap;
	HIP_TRY(hipMemsetAsync(ctx->d_counter, 0, sizeof(unsigned long long), s));
	const unsigned nwg	 = std::min(2048u, (unsigned) ctx->nbc);// the kernel strides over the blocks
	const Partition& P = ctx->part[ctx->rollid];
	if(tri_vel && cap)
		grid_isosurface_kernel<true><<<nwg, kIsoThreads, 0, s>>>(ctx->g, ctx->nbc, P.keys, P.table, ctx->grid[0], a, d_xyz.p, d_vel.p, ctx->d_counter);
	else
		grid_isosurface_kernel<false><<<nwg, kIsoThreads, 0, s>>>(ctx->g, ctx->nbc, P.keys, P.table, ctx->grid[0], a, d_xyz.p, nullptr, ctx->d_counter);
	HIP_TRY(hipGetLastError());
	unsigned long long count = 0;
	HIP_TRY(hipMemcpyAsync(&count, ctx->d_counter, sizeof(count), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const size_t got = (size_t) std::min<unsigned long long>(count, cap);
	if(got) {
		HIP_TRY(hipMemcpy(tri_xyz, d_xyz.p, sizeof(float) * 9 * got, hipMemcpyDeviceToHost));
		if(tri_vel) HIP_TRY(hipMemcpy(tri_vel, d_vel.p, sizeof(float) * 9 * got, hipMemcpyDeviceToHost));
	}
	*n = (size_t) count;
	if(tri_xyz && count > cap) return fail(ctx, MPM_ERR_CAPACITY, "mpm_grid_isosurface: the surface has " + std::to_string(count) + " triangles, the buffers hold " + std::to_string(cap));
	return MPM_OK;
}

// Collider loads (mpm_collider_loads.hpp): mpm_grid_volume's preconditions and dt > 0.  The one-shot calls stage in scratch released on every exit
// path; the gauge owns its two arrays while it is on, so a context that never asks allocates and launches nothing for any of this.
static int loads_state(mpm_ctx* ctx, float dt, const char* who) {
	if(!(dt > 0.f)) return fail(ctx, MPM_ERR_INVALID, std::string(who) + ": dt must be > 0");
	return readout_state(ctx, who);
}
int mpm_collider_loads(mpm_ctx* ctx, float dt, const mpm_load_options* opt, double out[MPM_LOAD_ROWS][8]) {
	static_assert(MPM_LOAD_ROWS == kLoadRows && kLoadSums == 8, "the ABI's rows are the kernels'");
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(!out) return fail(ctx, MPM_ERR_INVALID, "mpm_collider_loads: NULL out");
	if(int rc = loads_state(ctx, dt, "mpm_collider_loads")) return rc;
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	DevBuf<double> d_part, d_out;
	if(d_part.alloc((size_t) kLoadGroups * kLoadRows * kLoadSums, s) != hipSuccess || d_out.alloc(kLoadRows * kLoadSums, s) != hipSuccess) {
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_collider_loads: no device memory");
	}
	if(int rc = launch_collider_loads(ctx, dt, opt, d_part.p, d_out.p, 0, ctx->force)) return rc;
	HIP_TRY(hipMemcpyAsync(&out[0][0], d_out.p, sizeof(double) * kLoadRows * kLoadSums, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	return MPM_OK;
}

int mpm_collider_contacts(mpm_ctx* ctx, float dt, int32_t* node_row4, float* rec8, size_t* n) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(!n) return fail(ctx, MPM_ERR_INVALID, "mpm_collider_contacts: NULL n");
	if((node_row4 == nullptr) != (rec8 == nullptr)) return fail(ctx, MPM_ERR_INVALID, "mpm_collider_contacts: node_row4 and rec8 are given together or not at all");
	if(int rc = loads_state(ctx, dt, "mpm_collider_contacts")) return rc;
	const size_t cap = node_row4 ? *n : 0;
	if(cap > SIZE_MAX / (8 * sizeof(float))) return fail(ctx, MPM_ERR_CAPACITY, "mpm_collider_contacts: no device memory for " + std::to_string(cap) + " records");
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	DevBuf<int> d_nr;
	DevBuf<float> d_rec;
	if(cap && (d_nr.alloc(4 * cap, s) != hipSuccess || d_rec.alloc(8 * cap, s) != hipSuccess)) {
		(void) hipGetLastError();// (the context stays usable; *n is left as it was)
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_collider_contacts: no device memory for " + std::to_string(cap) + " records");
	}
	HIP_TRY(hipMemsetAsync(ctx->d_counter, 0, sizeof(unsigned long long), s));
	with_collider_at_clock(ctx, [&](const auto& col) {
		collider_contacts_kernel<<<kLoadGroups, 256, 0, s>>>(ctx->g, &ctx->d_status[ST_NBC], ctx->grid[0], ctx->part[ctx->rollid].keys, dt, col, (unsigned long long) cap, d_nr.p, d_rec.p, ctx->d_counter, ctx->force);
	});
	HIP_TRY(hipGetLastError());
	unsigned long long count = 0;
	HIP_TRY(hipMemcpyAsync(&count, ctx->d_counter, sizeof(count), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const size_t got = (size_t) std::min<unsigned long long>(count, cap);
	if(got) {
		HIP_TRY(hipMemcpy(node_row4, d_nr.p, sizeof(int32_t) * 4 * got, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(rec8, d_rec.p, sizeof(float) * 8 * got, hipMemcpyDeviceToHost));
	}
	*n = (size_t) count;
	if(node_row4 && count > cap) return fail(ctx, MPM_ERR_CAPACITY, "mpm_collider_contacts: there are " + std::to_string(count) + " records, the buffers hold " + std::to_string(cap));
	return MPM_OK;
}

int mpm_load_gauge(mpm_ctx* ctx, int on, const mpm_load_options* opt) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(on && (ctx->group_refs > 0 || ctx->mgsp_rank >= 0 || ctx->halo_tagged)) return fail(ctx, MPM_ERR_INVALID, "mpm_load_gauge: the context belongs (or belonged) to a multi-GPU group; group-wide loads are not computed");
	HIP_TRY(hipSetDevice(ctx->device));
	if(!on) {
		HIP_TRY(hipStreamSynchronize(ctx->s_compute));
		(void) ctx->d_load_partials.reset();
		(void) ctx->d_load_acc.reset();
		ctx->load_gauge = false;
		return MPM_OK;
	}
	if(!ctx->d_load_partials && ctx->d_load_partials.alloc((size_t) kLoadGroups * kLoadRows * kLoadSums, ctx->s_compute) != hipSuccess) {
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_load_gauge: no device memory");
	}
	if(!ctx->d_load_acc && ctx->d_load_acc.alloc(kLoadAccDoubles, ctx->s_compute) != hipSuccess) {
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_load_gauge: no device memory");
	}
	HIP_TRY(hipMemsetAsync(ctx->d_load_acc, 0, sizeof(double) * kLoadAccDoubles, ctx->s_compute));
	ctx->load_opt = opt ? *opt : mpm_load_options {};
	ctx->load_gauge = true;
	return MPM_OK;
}

int mpm_load_gauge_read(mpm_ctx* ctx, double out[MPM_LOAD_ROWS][8], double* elapsed, int* updates, int reset) {
	if(!ctx || !ctx->ready) return MPM_ERR_NOT_READY;
	if(!ctx->load_gauge) return fail(ctx, MPM_ERR_INVALID, "mpm_load_gauge_read: the gauge is off (mpm_load_gauge)");
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	double acc[kLoadAccDoubles];
	HIP_TRY(hipMemcpyAsync(acc, ctx->d_load_acc, sizeof(acc), hipMemcpyDeviceToHost, s));
	if(reset) HIP_TRY(hipMemsetAsync(ctx->d_load_acc, 0, sizeof(acc), s));
	HIP_TRY(hipStreamSynchronize(s));
	if(out) memcpy(&out[0][0], acc, sizeof(double) * kLoadRows * kLoadSums);
	if(elapsed) *elapsed = acc[kLoadRows * kLoadSums];
	if(updates) {
		long long count = 0;
		memcpy(&count, &acc[kLoadRows * kLoadSums + 1], sizeof(count));
		*updates = (int) std::min<long long>(count, INT32_MAX);
	}
	return MPM_OK;
}

// Rigid bodies (mpm_rigid_body.hpp).  Every check and every allocation comes before the first change: a refused call changes nothing.
static bool is_body(const mpm_ctx* ctx, int slot) {
	return slot_ok(slot) && ((ctx->body_mask >> slot) & 1);
}
static void fill_rigid_body(mpm_rigid_body* out, double mass, const double (&I6)[6], const double (&com)[3]) {
	*out	  = mpm_rigid_body {};
	out->mass = (float) mass;
	for(int i = 0; i < 6; ++i) out->inertia[i] = (float) I6[i];
	for(int d = 0; d < 3; ++d) out->com[d] = (float) com[d];
	out->gravity = 1;
}
int mpm_set_collider_body(mpm_ctx* ctx, int slot, const mpm_rigid_body* body) {
	static_assert(sizeof(mpm_rigid_body_state) == sizeof(BodyState) && offsetof(mpm_rigid_body_state, updates) == offsetof(BodyState, updates), "the ABI's state is the kernels'");
	if(!ctx) return MPM_ERR_INVALID;
	if(!slot_ok(slot)) return fail(ctx, MPM_ERR_INVALID, "mpm_set_collider_body: slot outside 0..3");
	HIP_TRY(hipSetDevice(ctx->device));
	hipStream_t s = ctx->s_compute;
	if(!body) {// prescribed again: at rest, at the pose the body has reached
		if(!is_body(ctx, slot)) return fail(ctx, MPM_ERR_INVALID, "mpm_set_collider_body: the slot holds no rigid body");
		BodyPose bp;
		HIP_TRY(hipStreamSynchronize(s));
		HIP_TRY(hipMemcpy(&bp, &ctx->d_body.p->pose[slot], sizeof(bp), hipMemcpyDeviceToHost));
		CollisionPose p = collision_pose(ctx->shape[slot].obj, 0.f);// (inv = 1, growth = 0)
		for(int i = 0; i < 9; ++i) p.rot[i] = bp.rot[i];
		for(int d = 0; d < 3; ++d) p.shift[d] = bp.shift[d];
		ctx->frozen_pose[slot] = p;
		ctx->frozen[slot]	   = true;
		ctx->body_mask &= ~(1 << slot);
		return MPM_OK;
	}
	if(ctx->group_refs > 0 || ctx->mgsp_rank >= 0 || ctx->halo_tagged) return fail(ctx, MPM_ERR_INVALID, "mpm_set_collider_body: the context belongs (or belonged) to a multi-GPU group; bodies in groups are not computed");
	const ShapeSlot& sl = ctx->shape[slot];
	const int kind		= sl.shape.kind;
	if(kind == 0) return fail(ctx, MPM_ERR_INVALID, "mpm_set_collider_body: the slot is empty");
	if(kind == kShapeHalfspace || kind == kShapeHeightfield) return fail(ctx, MPM_ERR_INVALID, "mpm_set_collider_body: a half-space or a heightfield is unbounded and cannot be a rigid body");
	for(int r: body->reserved)
		if(r) return fail(ctx, MPM_ERR_INVALID, "mpm_set_collider_body: reserved words must be 0");
	// where the collider stands now: a body, a slot released from one, or a prescribed collider at the clock's time
	CollisionPose now = ctx->frozen[slot] ? ctx->frozen_pose[slot] : collision_pose(sl.obj, ctx->collision.time);
	float v0[3] = {sl.obj.trans_vel[0], sl.obj.trans_vel[1], sl.obj.trans_vel[2]}, w0[3] = {sl.obj.omega[0], sl.obj.omega[1], sl.obj.omega[2]};
	const bool again = is_body(ctx, slot);// new constants for a body in motion: it keeps its float64 state (below); the checks see its float32 pose
	BodyState old {};
	if(again) {
		BodyPose bp;
		HIP_TRY(hipStreamSynchronize(s));
		HIP_TRY(hipMemcpy(&old, &ctx->d_body.p->st[slot], sizeof(old), hipMemcpyDeviceToHost));
		body_pose(old, bp);
		for(int i = 0; i < 9; ++i) now.rot[i] = bp.rot[i];
		for(int d = 0; d < 3; ++d) now.shift[d] = bp.shift[d], v0[d] = bp.vel[d], w0[d] = bp.omega[d];
	}
	if(const char* msg = body_object_ok(sl.obj.scale, sl.obj.dsdt, now.rot, sl.obj.trans, v0, w0)) return fail(ctx, MPM_ERR_INVALID, std::string("mpm_set_collider_body: ") + msg);
	BodyConst c;
	if(const char* msg = body_constants(body->mass, body->inertia, body->com, body->gravity, body->lock, body->force, body->torque, c)) return fail(ctx, MPM_ERR_INVALID, std::string("mpm_set_collider_body: ") + msg);
	BodyState st;
	body_start(now.rot, now.shift, sl.obj.trans, v0, w0, c, st);
	if(again) body_reconstant(old, ctx->body_c[slot], c, st);
	BodyPose pose;
	body_pose(st, pose);
	if((!ctx->d_body && ctx->d_body.alloc(1, s) != hipSuccess) || (!ctx->d_body_partials && ctx->d_body_partials.alloc((size_t) kLoadGroups * kLoadRows * kLoadSums, s) != hipSuccess)) {
		(void) hipGetLastError();
		return fail(ctx, MPM_ERR_CAPACITY, "mpm_set_collider_body: no device memory");
	}
	HIP_TRY(hipStreamSynchronize(s));
	HIP_TRY(hipMemcpy(&ctx->d_body.p->st[slot], &st, sizeof(st), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(&ctx->d_body.p->c[slot], &c, sizeof(c), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(&ctx->d_body.p->pose[slot], &pose, sizeof(pose), hipMemcpyHostToDevice));
	CollisionObject& o = ctx->shape[slot].obj;// re-pivoted to the centre of mass, without a velocity of its own: collision_respond's object velocity is exactly 0
	for(int d = 0; d < 3; ++d) o.trans[d] = body->com[d], o.trans_vel[d] = 0.f, o.omega[d] = 0.f;
	ctx->body_c[slot]	 = c;
	ctx->body_desc[slot] = *body;
	ctx->frozen[slot]	 = false;
	ctx->body_mask |= 1 << slot;
	return MPM_OK;
}

int mpm_get_collider_body(mpm_ctx* ctx, int slot, mpm_rigid_body* body_out, mpm_rigid_body_state* state_out) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!is_body(ctx, slot)) return fail(ctx, MPM_ERR_INVALID, "mpm_get_collider_body: the slot holds no rigid body");
	if(body_out) *body_out = ctx->body_desc[slot];
	if(state_out) {
		HIP_TRY(hipSetDevice(ctx->device));
		HIP_TRY(hipStreamSynchronize(ctx->s_compute));
		HIP_TRY(hipMemcpy(state_out, &ctx->d_body.p->st[slot], sizeof(BodyState), hipMemcpyDeviceToHost));
	}
	return MPM_OK;
}

int mpm_set_collider_body_state(mpm_ctx* ctx, int slot, const double position[3], const double orientation[4], const double velocity[3], const double omega[3]) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!is_body(ctx, slot)) return fail(ctx, MPM_ERR_INVALID, "mpm_set_collider_body_state: the slot holds no rigid body");
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipStreamSynchronize(ctx->s_compute));
	BodyState st;
	HIP_TRY(hipMemcpy(&st, &ctx->d_body.p->st[slot], sizeof(st), hipMemcpyDeviceToHost));
	if(const char* msg = body_restart(st, ctx->body_c[slot], position, orientation, velocity, omega)) return fail(ctx, MPM_ERR_INVALID, std::string("mpm_set_collider_body_state: ") + msg);
	BodyPose pose;
	body_pose(st, pose);
	HIP_TRY(hipMemcpy(&ctx->d_body.p->st[slot], &st, sizeof(st), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(&ctx->d_body.p->pose[slot], &pose, sizeof(pose), hipMemcpyHostToDevice));
	return MPM_OK;
}

int mpm_shape_mass_properties(const mpm_collision_shape* shape, float density, mpm_rigid_body* out) {
	if(!shape || !out) return MPM_ERR_INVALID;
	double mass, I6[6], com[3];
	if(body_shape_mass(shape->kind, shape->inside_out, shape->a, shape->b, shape->radius, (double) density, mass, I6, com)) return MPM_ERR_INVALID;
	fill_rigid_body(out, mass, I6, com);
	return MPM_OK;
}

int mpm_mesh_mass_properties(const float* verts, size_t nv, const int32_t* tris, size_t nt, float density, mpm_rigid_body* out) {
	if(!verts || !tris || !out) return MPM_ERR_INVALID;
	MeshRecords m;
	if(!m.build(verts, nv, tris, nt, 1.f).empty()) return MPM_ERR_INVALID;
	double mass, I6[6], com[3];
	if(body_mesh_mass(verts, nv, tris, nt, (double) density, mass, I6, com)) return MPM_ERR_INVALID;
	fill_rigid_body(out, mass, I6, com);
	return MPM_OK;
}

// ---- function-level tests ---------------------------------------------------------------------------
#define HIP_TRY0(expr)                      \
	do {                                       \
		if((expr) != hipSuccess) return MPM_ERR_DEVICE; \
	} while(0)

int mpm_test_eig(const float* F, size_t n, float* out12, int device) {
	if(!F || !out12 || n == 0) return MPM_ERR_INVALID;
	HIP_TRY0(hipSetDevice(device));
	DevBuf<float> dF, dO;
	HIP_TRY0(dF.alloc(9 * n, nullptr));
	HIP_TRY0(dO.alloc(12 * n, nullptr));
	HIP_TRY0(hipMemcpy(dF.p, F, sizeof(float) * 9 * n, hipMemcpyHostToDevice));
	test_eig_kernel<<<cdiv(n, 256), 256>>>(n, dF.p, dO.p);
	HIP_TRY0(hipGetLastError());
	HIP_TRY0(hipMemcpy(out12, dO.p, sizeof(float) * 12 * n, hipMemcpyDeviceToHost));
	return MPM_OK;
}

int mpm_test_stress(int material, const mpm_material_params* p, const float* F, const float* logjp, size_t n, float* out19, int device) {
	if(material < 1 || material > 3 || !p) return MPM_ERR_INVALID;
	HIP_TRY0(hipSetDevice(device));
	DevBuf<float> dF, dL, dO;
	HIP_TRY0(dF.alloc(9 * n, nullptr));
	HIP_TRY0(dO.alloc(19 * n, nullptr));
	HIP_TRY0(hipMemcpy(dF.p, F, sizeof(float) * 9 * n, hipMemcpyHostToDevice));
	if(logjp) {
		HIP_TRY0(dL.alloc(n, nullptr));
		HIP_TRY0(hipMemcpy(dL.p, logjp, sizeof(float) * n, hipMemcpyHostToDevice));
	}
	test_stress_kernel<<<cdiv(n, 256), 256>>>(material, make_material_const(*p), n, dF.p, dL.p, dO.p, nullptr);
	HIP_TRY0(hipGetLastError());
	HIP_TRY0(hipMemcpy(out19, dO.p, sizeof(float) * 19 * n, hipMemcpyDeviceToHost));
	return MPM_OK;
}

// The shared half of the three collider queries below: points up, test_collision_query_kernel, four floats per point down
static int test_collision_query(ShapeSlot c, const Heightfield& f, float time, const float* xyz, size_t n, float* out4, const Volume& vol = Volume {}) {
	c.pose = collision_pose(c.obj, time);
	DevBuf<float> dX, dO;
	HIP_TRY0(dX.alloc(3 * n, nullptr));
	HIP_TRY0(dO.alloc(4 * n, nullptr));
	HIP_TRY0(hipMemcpy(dX.p, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
	test_collision_query_kernel<<<cdiv(n, 256), 256>>>(c, f, vol, n, dX.p, dO.p);
	HIP_TRY0(hipGetLastError());
	HIP_TRY0(hipMemcpy(out4, dO.p, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
	return MPM_OK;
}

int mpm_test_collision_shape(const mpm_collision_object* obj, const mpm_collision_shape* shape, float time, float dx, const float* xyz, size_t n, float* out4, int device) {
	(void) dx;// (positions are domain points already; kept for the call shape of the grid kernels)
	if(!obj || !shape || !xyz || !out4 || n == 0) return MPM_ERR_INVALID;
	ShapeSlot c {};
	if(make_shape_slot(obj, shape, c)) return MPM_ERR_INVALID;
	HIP_TRY0(hipSetDevice(device));
	return test_collision_query(c, Heightfield {}, time, xyz, n, out4);
}

int mpm_test_collision_heightfield(const mpm_collision_object* obj, const mpm_heightfield* hf, const float* heights, float time, const float* xyz, size_t n, float* out4, int device) {
	if(!obj || !hf || !heights || !xyz || !out4 || n == 0) return MPM_ERR_INVALID;
	ShapeSlot c {};
	Heightfield f {};
	if(make_heightfield_slot(obj, hf, c, f)) return MPM_ERR_INVALID;
	const size_t cells = (size_t) f.nx * f.nz;
	std::vector<float4> table(cells);
	if(!heightfield_build(heights, f.nx, f.nz, f.spacing, table.data())) return MPM_ERR_INVALID;
	HIP_TRY0(hipSetDevice(device));
	DevBuf<float4> dT;
	HIP_TRY0(dT.alloc(cells, nullptr));
	HIP_TRY0(hipMemcpy(dT.p, table.data(), sizeof(float4) * cells, hipMemcpyHostToDevice));
	f.table = dT.p;
	return test_collision_query(c, f, time, xyz, n, out4);
}

int mpm_test_collision_volume(const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* field4, float time, const float* xyz, size_t n, float* out4, int device) {
	if(!obj || !vol || !field4 || !xyz || !out4 || n == 0) return MPM_ERR_INVALID;
	ShapeSlot c {};
	Volume v {};
	if(make_volume_slot(obj, vol, false, c, v)) return MPM_ERR_INVALID;
	const size_t cells = (size_t) v.dims[0] * (size_t) v.dims[1] * (size_t) v.dims[2];
	if(!volume_samples_finite(field4, cells)) return MPM_ERR_INVALID;
	HIP_TRY0(hipSetDevice(device));
	DevBuf<float4> dT;
	HIP_TRY0(dT.alloc(cells, nullptr));
	HIP_TRY0(hipMemcpy(dT.p, field4, sizeof(float4) * cells, hipMemcpyHostToDevice));
	v.table = dT.p;
	return test_collision_query(c, Heightfield {}, time, xyz, n, out4, v);
}

// Force fields ------------------------------------------------------------------------------------------------------------------------------
// mpm_force_field -> the slot the kernels read (the vortex axis and a half-space region's normal normalised; fields a kind does not read are
// kept as given); nullptr, or the message that names the offending field
static const char* make_force_slot(const mpm_force_field* f, ForceSlot& out) {
	if(f->kind < MPM_FORCE_UNIFORM || f->kind > MPM_FORCE_DRAG) return "force field: unknown kind";
	if(f->falloff < 0 || f->falloff > 2) return "force field: falloff outside 0..2";
	for(int w: f->reserved)
		if(w) return "force field: a reserved word is not 0";
	if(!shape_finite3(f->vec)) return "force field: vec is not finite";
	if(!shape_finite3(f->centre)) return "force field: centre is not finite";
	if(!std::isfinite(f->strength)) return "force field: strength is not finite";
	if(!std::isfinite(f->swirl) || !std::isfinite(f->pull) || !std::isfinite(f->lift)) return "force field: swirl, pull or lift is not finite";
	if(!std::isfinite(f->soft) || f->soft < 0.f) return "force field: soft must be finite and >= 0";
	if(!std::isfinite(f->feather) || f->feather < 0.f) return "force field: feather must be finite and >= 0";
	if(f->kind == MPM_FORCE_DRAG && f->strength < 0.f) return "force field: strength of a DRAG field must be >= 0";
	ForceSlot c {};
	c.kind	  = f->kind;
	c.falloff = f->falloff;
	for(int d = 0; d < 3; ++d) c.vec[d] = f->vec[d], c.centre[d] = f->centre[d];
	if(f->kind == MPM_FORCE_VORTEX) {
		const float len = sqrtf(f->vec[0] * f->vec[0] + f->vec[1] * f->vec[1] + f->vec[2] * f->vec[2]);
		if(!(len > 0.f) || !std::isfinite(len)) return "force field: the axis vec of a VORTEX field must not be zero";
		for(int d = 0; d < 3; ++d) c.vec[d] = f->vec[d] / len;// (a unit axis stays exactly itself)
	}
	c.strength = f->strength, c.swirl = f->swirl, c.pull = f->pull, c.lift = f->lift, c.soft = f->soft, c.feather = f->feather;
	if(f->region.kind) {
		const mpm_collision_shape& r = f->region;
		if(!shape_finite3(r.a) || !std::isfinite(r.radius) || (r.kind != MPM_SHAPE_SPHERE && !shape_finite3(r.b))) return "force field: region: a number is not finite";
		mpm_collision_object obj;
		mpm_default_collision_object(&obj);
		ShapeSlot slot;
		if(const char* msg = make_shape_slot(&obj, &r, slot)) return msg;// ("collision shape: ...": the region's own field)
		c.region = slot.shape;
	}
	out = c;
	return nullptr;
}
static bool force_slot_ok(int slot) {
	return slot >= 0 && slot < MPM_MAX_FORCE_FIELDS;
}

int mpm_set_force_field(mpm_ctx* ctx, int slot, const mpm_force_field* f) {
	static_assert(MPM_MAX_FORCE_FIELDS == kMaxForceFields && MPM_FORCE_DRAG == kForceDrag, "the ABI's kinds and slots are the kernels'");
	if(!ctx) return MPM_ERR_INVALID;
	if(!force_slot_ok(slot)) return fail(ctx, MPM_ERR_INVALID, "mpm_set_force_field: slot outside 0..3");
	ForceSlot c {};
	if(f) {
		if(const char* msg = make_force_slot(f, c)) return fail(ctx, MPM_ERR_INVALID, std::string("mpm_set_force_field: ") + msg);
		if(ctx->group_refs > 0 || ctx->mgsp_rank >= 0 || ctx->halo_tagged)
			return fail(ctx, MPM_ERR_INVALID, "mpm_set_force_field: the context belongs (or belonged) to a multi-GPU group; force fields in groups are not computed");
		if(ctx->grid_preupdated) return fail(ctx, MPM_ERR_INVALID, "mpm_set_force_field: the next grid update has been applied already: install at a substep boundary");
	}
	ctx->force.slot[slot] = c;// (kind 0: empty.  By value with the next launch: nothing enqueued reads it)
	ctx->force.count	  = 0;
	for(int i = 0; i < kMaxForceFields; ++i)
		if(ctx->force.slot[i].kind) ctx->force.count = i + 1;
	return MPM_OK;
}

int mpm_get_force_field(mpm_ctx* ctx, int slot, mpm_force_field* out) {
	if(!ctx) return MPM_ERR_INVALID;
	if(!force_slot_ok(slot)) return fail(ctx, MPM_ERR_INVALID, "mpm_get_force_field: slot outside 0..3");
	if(!out) return fail(ctx, MPM_ERR_INVALID, "mpm_get_force_field: NULL out");
	const ForceSlot& c = ctx->force.slot[slot];
	mpm_force_field o {};
	o.kind = c.kind, o.falloff = c.falloff;
	for(int d = 0; d < 3; ++d) o.vec[d] = c.vec[d], o.centre[d] = c.centre[d], o.region.a[d] = c.region.a[d], o.region.b[d] = c.region.b[d];
	o.strength = c.strength, o.swirl = c.swirl, o.pull = c.pull, o.lift = c.lift, o.soft = c.soft, o.feather = c.feather;
	o.region.kind = c.region.kind, o.region.inside_out = c.region.inside_out, o.region.radius = c.region.radius;
	*out = o;
	return MPM_OK;
}

int mpm_test_force_field(const mpm_force_field* fields, int n_fields, float dt, float dx, const float* xyz, const float* mp4, size_t n, float* out4, int device) {
	(void) dx;// (positions are domain points already; kept for the call shape of the grid kernels)
	if(n_fields < 0 || n_fields > MPM_MAX_FORCE_FIELDS || (n_fields && !fields)) return MPM_ERR_INVALID;
	ForceArgs fa {};
	for(int i = 0; i < n_fields; ++i) {
		if(fields[i].kind == 0) continue;
		if(make_force_slot(&fields[i], fa.slot[i])) return MPM_ERR_INVALID;
		fa.count = i + 1;
	}
	if(!xyz || !mp4 || !out4 || n == 0) return MPM_ERR_INVALID;
	HIP_TRY0(hipSetDevice(device));
	DevBuf<float> dX, dM, dO;
	HIP_TRY0(dX.alloc(3 * n, nullptr));
	HIP_TRY0(dM.alloc(4 * n, nullptr));
	HIP_TRY0(dO.alloc(4 * n, nullptr));
	HIP_TRY0(hipMemcpy(dX.p, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
	HIP_TRY0(hipMemcpy(dM.p, mp4, sizeof(float) * 4 * n, hipMemcpyHostToDevice));
	test_force_field_kernel<<<cdiv(n, 256), 256>>>(fa, dt, n, dX.p, dM.p, dO.p);
	HIP_TRY0(hipGetLastError());
	HIP_TRY0(hipMemcpy(out4, dO.p, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
	return MPM_OK;
}

int mpm_streams(mpm_ctx* ctx, void** compute_stream, void** comm_stream) {
	if(!ctx) return MPM_ERR_INVALID;
	if(compute_stream) *compute_stream = (void*) ctx->s_compute;
	if(comm_stream) *comm_stream = (void*) ctx->s_comm;
	return MPM_OK;
}

int mpm_sync(mpm_ctx* ctx) {
	if(!ctx) return MPM_ERR_INVALID;
	HIP_TRY(hipSetDevice(ctx->device));
	HIP_TRY(hipStreamSynchronize(ctx->s_compute));
	HIP_TRY(hipStreamSynchronize(ctx->s_comm));
	return MPM_OK;
}

}// extern "C"

#include "mpm_halo.inc"
#include "mpm_checkpoint.inc"
#include "mpm_group.inc"
