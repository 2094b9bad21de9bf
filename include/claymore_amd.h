/*
 * claymore_amd.h — C ABI of the MI355X-native MPM substep engine (libclaymore_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of penn-graphics-research/claymore:
 *     grid update -> fused G2P2G -> sparse block-partition rebuild      (Projects/GMPM)
 *     + static-particle-partition halo exchange                          (Projects/MGSP)
 * The reference has no FFI layer: its kernels are C++ templates launched through
 * Cuda::CudaContext::compute_launch (Library/MnSystem/Cuda/Cuda.h:151-184) from the two host classes
 * GmpmSimulator (Projects/GMPM/gmpm_simulator.cuh) and MgspBenchmark (Projects/MGSP/mgsp_benchmark.cuh).
 * Each entry point below replaces one phase of those classes; the file:line it replaces is cited.
 *
 * Conventions
 *   - plain C, POD structs, caller-owned host arrays are copied during the call, the context owns
 *     every device buffer (reference: members of GmpmSimulator, gmpm_simulator.cuh:96-141);
 *   - every function returns an mpm_status (0 = ok); mpm_last_error() gives the text.  The reference
 *     prints and exit()s (Library/MnSystem/Cuda/HostUtils.hpp:33-44) or abort()s on capacity overflow
 *     (gmpm_simulator.cuh:473-476); host drivers map a non-zero status to that behaviour;
 *   - a context is bound to one HIP device and is single-thread-affine (reference: one worker thread
 *     per GPU, mgsp_benchmark.cuh:309-334);
 *   - there is NO CPU fallback behind this ABI: if no HIP device is usable, mpm_create fails.
 *
 * The CPU oracle (oracle/, test infrastructure only) exports the same functions with the prefix
 * mpmo_ instead of mpm_ so that tests can drive both through identical call sequences.
 */
#ifndef CLAYMORE_AMD_H
#define CLAYMORE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mpm_status {
	MPM_OK			   = 0,
	MPM_ERR_INVALID	   = 1, /* bad argument / call order */
	MPM_ERR_DEVICE	   = 2, /* HIP runtime error (reference: check_cuda_errors -> exit) */
	MPM_ERR_CAPACITY   = 3, /* block / bin / cell capacity exceeded (reference: std::abort) */
	MPM_ERR_NONFINITE  = 4, /* inf/NaN grid velocity (reference: stops main loop, gmpm_simulator.cuh:355-358) */
	MPM_ERR_NOT_READY  = 5,
	MPM_ERR_INTERNAL   = 6 /* the library's own books do not balance: particles bucketed + lost + dropped != particles added (the reference
							  only prints the total per frame, gmpm_simulator.cuh:617); the message names the model */
} mpm_status;

/* Projects/GMPM/settings.h:20-26 */
typedef enum mpm_material {
	MPM_J_FLUID			= 0,
	MPM_FIXED_COROTATED = 1,
	MPM_SAND			= 2,
	MPM_NACC			= 3
} mpm_material;

/* Runtime replacement of the compile-time config:: constants (Projects/GMPM/settings.h:33-96). */
typedef struct mpm_config {
	int domain_bits;	 /* grid = 2^bits cells per axis on [0,1)^3; settings.h:59 DOMAIN_BITS (7..10) */
	int max_ppc;		 /* particles per cell capacity; settings.h:75 (reference 128); power of two <= 128 */
	int boundary_blocks; /* slip-wall zone in blocks; settings.h:63 G_BOUNDARY_CONDITION = 2 */
	float gravity;		 /* settings.h:85 (-9.8; MGSP settings.h:108 uses -4.9) */
	float cfl;			 /* utility_funcs.hpp:41 uses 0.5 (MGSP utility_funcs.hpp:39: 0.3) */
	int64_t max_blocks;	 /* (initial) capacity in (exterior) blocks; settings.h:89 G_MAX_ACTIVE_BLOCK; 0 = size from the models */
	int grow;			 /* 1 (default): block / bin capacities grow by 3/2 once 3/4 full, like check_capacity()
							(gmpm_simulator.cuh:283-300); 0: fixed capacities, MPM_ERR_CAPACITY when exceeded */
	int drop_overflow;	 /* 0 (default): a block receiving more than max_ppc * 64 particles is MPM_ERR_CAPACITY; 1: the particles beyond the
							capacity are dropped and counted (mpm_diagnostics.dropped_particles) - what the reference does, silently and
							per cell (particle_buffer.cuh:122-130) */
	int sync_interval;	 /* mpm_run_fixed: substeps enqueued between two host synchronisations (the kernels read their block counts from
							device memory; errors raised in between are reported at the next synchronisation).  0 = default (8), 1 = one
							synchronisation per substep.  The reference synchronises six times per substep (gmpm_simulator.cuh:398-564) */
	int still_rebuild;	 /* mpm_run_fixed on a single context: a substep in which no particle changed its block keeps the partition as it is
							(same blocks under the same numbers) instead of rebuilding it.  0 = default = on, -1 = off.  HIP library only */
	int reserved[2];
} mpm_config;

/* Material parameter block (Projects/GMPM/particle_buffer.cuh:141-264).  Unused fields are ignored. */
typedef struct mpm_material_params {
	float rho;			  /* density; mass = rho * volume (particle_buffer.cuh:155-162) */
	float volume;		  /* particle volume */
	float youngs_modulus; /* FC / SAND / NACC */
	float poisson_ratio;
	float bulk;		 /* J_FLUID */
	float gamma;	 /* J_FLUID */
	float viscosity; /* J_FLUID */
	float beta;		 /* SAND (1.0) / NACC (0.5) */
	float xi;		 /* NACC hardening factor */
	float cohesion;	 /* SAND */
	float yield_surface;   /* SAND */
	float msqr;			   /* NACC */
	float log_jp0;		   /* SAND 0, NACC -0.01 */
	int volume_correction; /* SAND */
	int hardening_on;	   /* NACC */
	int reserved[5];
} mpm_material_params;

/* Block / bin counts after a rebuild (gmpm_simulator.cuh:572-575 prints exactly these). */
typedef struct mpm_counts {
	int particle_blocks; /* partition_block_count */
	int neighbor_blocks; /* neighbor_block_count  */
	int exterior_blocks; /* exterior_block_count  */
	int model_count;
	int64_t bins[8];	  /* per model, bincount[i] */
	int64_t particles[8]; /* per model, particles currently bucketed */
} mpm_counts;

/* Per-phase device time of the most recent substep, in milliseconds (reference CudaTimer tags,
 * gmpm_simulator.cuh:346,400,507,526,543,576). */
typedef struct mpm_timers {
	float grid_update_ms;
	float g2p2g_ms;
	float partition_ms;
	float halo_ms;
	float total_ms;
	float reserved[3];
} mpm_timers;

typedef struct mpm_ctx mpm_ctx;

/* Fill cfg with the reference defaults for a grid resolution (settings.h). */
int mpm_default_config(int domain_bits, mpm_config* cfg);
/* Fill p with the reference defaults for a material at a resolution (particle_buffer.cuh:144-264;
 * note the FIXED_COROTATED and SAND default volume carries the reference's 10x factor, :176,:203). */
int mpm_default_material(int material, int domain_bits, mpm_material_params* p);

/* GmpmSimulator::GmpmSimulator + initialize (gmpm_simulator.cuh:121-166), Cuda::Cuda (Cuda.cu:28-137). */
int mpm_create(const mpm_config* cfg, int device, mpm_ctx** out);
void mpm_destroy(mpm_ctx* ctx);
const char* mpm_last_error(const mpm_ctx* ctx);

/* init_model<M> + update_*_parameters (gmpm_simulator.cuh:168-254). xyz = n*3 floats (host). Returns the
 * model index through *model_id. */
int mpm_add_model(mpm_ctx* ctx, int material, const mpm_material_params* params, const float* xyz, size_t n, const float v0[3], int* model_id);

/* initial_setup (gmpm_simulator.cuh:637-781): activate blocks, bucket particles, fill bins, build the
 * neighbor/exterior partition, rasterize the initial grid. */
int mpm_initial_setup(mpm_ctx* ctx);

/* Grid-update phase (gmpm_simulator.cuh:326-347; kernel mgmpm_kernels.cuh:325-420).  *max_vel_sqr receives
 * max |v|^2 over grid nodes (inf if a NaN was seen). */
int mpm_grid_update(mpm_ctx* ctx, float dt, float* max_vel_sqr);
/* compute_dt (utility_funcs.hpp:36-49) with this context's dx and CFL. */
float mpm_compute_dt(const mpm_ctx* ctx, float max_vel, float cur_time, float next_time, float dt_default);
/* G2P2G phase (gmpm_simulator.cuh:364-413; kernel mgmpm_kernels.cuh:665-937). */
int mpm_g2p2g(mpm_ctx* ctx, float dt, float next_dt);
/* Partition rebuild (gmpm_simulator.cuh:415-579), ends with the double-buffer roll. counts may be NULL. */
int mpm_rebuild_partition(mpm_ctx* ctx, mpm_counts* counts);

/* One whole substep = grid update, host dt, g2p2g, rebuild (the body of the loop gmpm_simulator.cuh:324-580).
 * dt is the current step; *next_dt = compute_dt(sqrt(max|v|^2), step_time, frame_time, dt_default). */
int mpm_substep(mpm_ctx* ctx, float dt, float step_time, float frame_time, float dt_default, float* next_dt, float* max_vel);
/* n substeps with a fixed dt (next_dt = dt): the loop of gmpm_simulator.cuh:324-580 without its host logic.  The substeps are enqueued
 * mpm_config.sync_interval at a time; between two host synchronisations every kernel reads its block counts from device memory.  A capacity
 * overflow or a non-finite velocity raised inside a window is reported when the window ends (the context is then in an undefined state, as
 * after any error of a run: load a checkpoint or destroy it).  Timers: per-substep averages over the call. */
int mpm_run_fixed(mpm_ctx* ctx, int nsteps, float dt);

/* output_model (gmpm_simulator.cuh:594-634; kernel mgmpm_kernels.cuh:1087-1122): positions of a model, order
 * unspecified.  *n: in = capacity of xyz in particles, out = particles written. */
int mpm_retrieve_positions(mpm_ctx* ctx, int model, float* xyz, size_t* n);
/* Extension used by the parity tests: also the per-particle state, same order as xyz.
 * state9: for FC/SAND/NACC the left Cauchy-Green tensor b = F F^T (symmetric 3x3, 9 floats) - the state this engine carries
 * instead of the reference's F: every model on the path is isotropic, so positions, grid and log Jp depend on F only through b
 * (claymore_amd/csrc/mpm_device_math.hpp); a negative state9[9*i] marks a reflected F (det F < 0, |.| is b00) -, or J in
 * state9[9*i] for J_FLUID; logjp may be NULL.  The reference itself retrieves positions only (mgmpm_kernels.cuh:1087-1122). */
int mpm_retrieve_state(mpm_ctx* ctx, int model, float* xyz, float* state9, float* logjp, size_t* n);
/* What state9 of mpm_retrieve_state holds for the solid models.  Until ABI 4 this library returned the deformation gradient F there
 * (what the CPU oracle's mpmo_retrieve_state still returns); since ABI 5 it returns b = F F^T, from which F cannot be recovered (the
 * rotation part of F never reaches an output of this path).  A caller written against the older meaning asks here instead of guessing;
 * mpm_build_info() carries the same fact as "state=b" and the ABI number. */
enum { MPM_STATE_F = 0, MPM_STATE_B = 1 };
int mpm_state_kind(void);
/* Extension (the reference has no velocity output): per-particle velocity of a model, read out from the grid the last call left
 * behind - the mass m_i and momentum p_i of each node after the last P2G - with the APIC gather of G2P at the particle's position:
 *   v_i = p_i / m_i for m_i > 0, else 0.  This is the state BEFORE the next grid update: gravity, walls and the collision object
 *         are not applied;
 *   vel[3*i..]     v_p = sum_i w_ip v_i over the 27-node quadratic B-spline stencil (base node, weights and tie rule of G2P);
 *   affine9[9*i..] C_p = D^-1 sum_i w_ip v_i (x_i - x_p)^T, D^-1 = 4 / dx^2, column-major like G2P2G's (affine9[9*i + 3*c + r] = C_rc);
 *                  may be NULL.
 * A node outside [0, 4G)^3 or in a block that is not registered holds nothing (v_i = 0); particles of cells -2 / -1 use the wrapped
 * stencil key of G2P.  xyz, vel and affine9 share one order (unspecified, as for mpm_retrieve_positions);
 * *n: in = capacity in particles, out = particles written.
 * Precondition: the grid holds momenta, which is the case after mpm_initial_setup, mpm_rebuild_partition, mpm_substep and mpm_run_fixed and
 * after loading a checkpoint saved in that state.  mpm_grid_update turns the momenta into velocities in place; between it and the next
 * mpm_rebuild_partition (mpm_g2p2g included) the readout is refused with MPM_ERR_INVALID.
 * Errors: MPM_ERR_NOT_READY before mpm_initial_setup; MPM_ERR_INVALID for a bad model, a NULL xyz / vel / n, a grid that holds velocities
 * (above), or a context that has ever joined an mpm_group or been through the halo tagging - the refusal is permanent for that context: its
 * grid holds the group's summed momentum only at the return of a group call, which the group readout tracks (mpm_group_retrieve_velocity
 * below; after a phase-level call it may hold only this rank's share of the halo nodes); MPM_ERR_CAPACITY when
 * *n is too small (the first *n particles are written).  mpm_last_error says which.  HIP library only. */
int mpm_retrieve_velocity(mpm_ctx* ctx, int model, float* xyz, float* vel, float* affine9, size_t* n);
/* Extension: the totals of the same readout without per-particle output, summed on the device in float64:
 *   out[0] = particle count, out[1..3] = sum_p m_p v_p, out[4] = sum_p 1/2 m_p |v_p|^2, m_p = volume * rho of the particle's model
 *   (the mass the set-up P2G uses).  model = -1: all models.  Preconditions and errors those of mpm_retrieve_velocity (a NULL out is
 *   MPM_ERR_INVALID).  The order of the device's float64 additions is unspecified: the last bits may differ between calls. */
int mpm_particle_momentum(mpm_ctx* ctx, int model, double out[5]);
/* Extension (the reference has no stress output): what the material of a model is doing, per particle, evaluated from the stored state -
 * b = F F^T with the sign of b00 marking a reflected F, and log Jp where the model has one (FC / SAND / NACC); J (J_FLUID).
 *   tau (solids)  = P F^T per unit reference volume: the model's compute_stress on the stored state with a zero velocity gradient, by the
 *                   device functions of the substep (claymore_amd/csrc/mpm_device_math.hpp, 2 mu / lambda unscaled).  SAND and NACC apply
 *                   their return mapping to the stored state as a substep would; the projected b and log Jp are discarded (the readout
 *                   writes no particle state), and tau and J are those of the projected state.
 *   J (solids)    = det F from the principal stretches that produced tau (product of sigma_k = sqrt(lambda_k(b)), negative for a reflected
 *                   F; SAND / NACC: of the projected stretches).
 *   J_FLUID       p = bulk (J^-gamma - 1), sigma = -p I, tau = J sigma.  The viscous part is NOT included: it is
 *                   viscosity (C_p + C_p^T) of mpm_retrieve_velocity's affine9, which needs the grid and has that call's preconditions.
 *   stress6[6*i..]  the Cauchy stress sigma = tau / J in the order {xx, yy, zz, xy, xz, yz}; may be NULL.
 *   scalars3[3*i..] {J, pressure = -tr sigma / 3, von Mises q = sqrt(3/2 dev sigma : dev sigma)}; may be NULL.
 * xyz, stress6 and scalars3 share one order (unspecified); xyz is bit-identical to what mpm_retrieve_state returns for the same particle, so
 * two readouts can be joined on the position bits.  *n: in = capacity in particles, out = particles written.
 * Preconditions: those of mpm_retrieve_state - any context after set-up, member of a group or not, at any substep boundary, whatever the
 * grid holds.  Errors: MPM_ERR_NOT_READY before mpm_initial_setup; MPM_ERR_INVALID for a bad model or a NULL xyz / n; MPM_ERR_CAPACITY
 * when *n is too small (the first *n particles are written).  HIP library only. */
int mpm_retrieve_stress(mpm_ctx* ctx, int model, float* xyz, float* stress6, float* scalars3, size_t* n);
/* The totals of the same evaluation without per-particle output, reduced on the device:
 *   out[0] = particle count, out[1..6] = sum_p V0 tau_p = sum_p V_p sigma_p in the order of stress6 (V0 = the model's `volume`; float64
 *   sums), out[7] = max_p q (exactly the largest q mpm_retrieve_stress reports).  model = -1: all models.  Preconditions and errors those
 *   of mpm_retrieve_stress (a NULL out is MPM_ERR_INVALID).  The order of the float64 additions is unspecified: the last bits of
 *   out[1..6] may differ between calls. */
int mpm_stress_totals(mpm_ctx* ctx, int model /* -1: all */, double out[8]);

int mpm_get_counts(mpm_ctx* ctx, mpm_counts* counts);

/* Full-state checkpoint / restart at a substep boundary (the reference has no restart: its only
 * output is output_model's position dump, gmpm_simulator.cuh:594-634).  The buffer holds both partitions' key lists, the
 * grid, and per model the bins, bin offsets, block sizes and packed advection lists.  mpm_checkpoint_load needs a context
 * with the same configuration and models that has been through mpm_initial_setup; capacities grow as needed.  After a
 * load the MGSP halo tags must be recomputed.  HIP library only. */
int mpm_checkpoint_size(mpm_ctx* ctx, size_t* bytes);
int mpm_checkpoint_save(mpm_ctx* ctx, void* buf, size_t capacity, size_t* written);
int mpm_checkpoint_load(mpm_ctx* ctx, const void* buf, size_t bytes);

/* Extension (the reference has no particle identity): a persistent 32-bit id per particle.  Every per-particle output of this engine comes
 * back in an unspecified order that changes from call to call; a tracked context can say which input particle a row is.
 *   id   the particle's index in the xyz array its model was given to mpm_add_model: 0 .. n-1 per model (for a group's ranks: each rank's
 *        ids index that rank's own arrays).  An id lives as long as its particle: lost, dropped and overflow-dropped particles take theirs
 *        with them, and the ids present are always distinct.
 * mpm_track_particle_ids switches tracking on (on != 0) or off; callable between mpm_create and mpm_initial_setup, MPM_ERR_INVALID after
 * set-up.  The default is off, and an untracked context allocates, launches and computes nothing more than before.  A tracked one carries
 * 2 x 4 B per bin slot and moves the ids with a small kernel beside every G2P2G launch.
 * mpm_retrieve_ids returns the positions and the id of every bucketed particle of a model in one shared order (unspecified).  xyz is
 * bit-identical to what mpm_retrieve_state returns for the same particle, so every other readout can be joined to the ids on the position
 * bits.  *n: in = capacity in particles, out = particles written.  Preconditions and errors: those of mpm_retrieve_state, and
 * MPM_ERR_INVALID for a NULL ids, for a context that does not track, and for ids that are not valid (below).
 * Ids, like colliders, are not part of the checkpoint buffer; their companion blob is: a header {uint64 magic "MPMPIDS1", int32 model count,
 * int32 0, then for each of 8 models int64 n, int64 bincount_src}, then per model one int32 per slot of the source bins (64 per bin,
 * bincount_src bins), in the slot order of the checkpoint's bins section.  Slots that hold no live particle carry an unspecified value on
 * save and are ignored on load.  mpm_checkpoint_load on a tracked context marks the ids invalid; mpm_retrieve_ids and
 * mpm_particle_ids_save then refuse until mpm_particle_ids_load succeeds.  The load validates the header against the context's current
 * state - the model count and every model's n and bincount_src - and refuses with MPM_ERR_INVALID otherwise: load the checkpoint first,
 * then the ids saved with it.  HIP library only. */
int mpm_track_particle_ids(mpm_ctx* ctx, int on);
int mpm_retrieve_ids(mpm_ctx* ctx, int model, float* xyz, int32_t* ids, size_t* n);
int mpm_particle_ids_size(mpm_ctx* ctx, size_t* bytes);
int mpm_particle_ids_save(mpm_ctx* ctx, void* buf, size_t capacity, size_t* written);
int mpm_particle_ids_load(mpm_ctx* ctx, const void* buf, size_t bytes);

/* Level-set collision object of the MGSP grid update (Projects/MGSP/boundary_condition.cuh:25-250, the second
 * update_grid_velocity_query_max overload Projects/MGSP/mgmpm_kernels.cuh:323-399, set up by
 * MgspBenchmark::init_boundary mgsp_benchmark.cuh:257-266).  Field values of SignedDistanceGrid. */
enum { MPM_BOUNDARY_STICKY = 0, MPM_BOUNDARY_SLIP = 1, MPM_BOUNDARY_SEPARATE = 2 }; /* BoundaryT, boundary_condition.cuh:19-23 */
typedef struct mpm_collision_object {
	int type;			/* BoundaryT; default STICKY (:46) */
	float friction;		/* 0.3 (:45) */
	float scale;		/* 1 (:44) */
	float dsdt;			/* 0 (:43) */
	float trans[3];		/* 0 */
	float trans_vel[3]; /* 0 */
	float omega[3];		/* 0 */
	float rot_mat[9];	/* identity; stored as the reference stores vec3x3: element (i, j) at [3 i + j] */
	float time;			/* `current_time` handed to detect_and_resolve_collision; the reference passes 0.f (:364).  Installing the
						 * object sets its clock to this value, stopped: see mpm_set_collision_clock */
	int reserved[3];
} mpm_collision_object;
int mpm_default_collision_object(mpm_collision_object* obj);
/* Install (obj != NULL) or remove (obj == NULL) the collision object.  sdf / grad_x / grad_y / grad_z: one float per grid
 * NODE of the whole domain, N = 2^domain_bits per axis, node (i, j, k) at [(i N + j) N + k] - the layout of the
 * reference's `<name>_sdf.bin` / `_grad_{0,1,2}.bin` files (boundary_condition.cuh:252-321).  Copied during the call.
 * With an object installed, mpm_grid_update follows the reference's boundary overload, including its max-velocity
 * quirk (|v|^2 is accumulated twice, mgmpm_kernels.cuh:365-373). */
int mpm_set_collision_object(mpm_ctx* ctx, const mpm_collision_object* obj, const float* sdf, const float* grad_x, const float* grad_y, const float* grad_z);
/* The object's clock: a moving object (trans_vel, omega, dsdt, start orientation rot_mat).  The pose is evaluated at the current
 * time T as the reference's detect_and_resolve_collision(..., current_time, ...) does: shape at trans + trans_vel T, turned by
 * rot_mat x Rx(omega_x T) x Ry(omega_y T) x Rz(omega_z T), grown by 1 + dsdt T.  A stopped clock (what mpm_set_collision_object
 * leaves behind) gives the surface its velocity while the shape stands still.
 * running = 1: the time advances by dt with every grid update of this context; running = 0: it stays at `time`.  Sets the current
 * time to `time` either way.  MPM_ERR_INVALID without an installed object; installing or removing an object stops the clock.
 * Rule: the grid update of a substep of length dt evaluates the object at T, the start of the substep, then T = T + dt in one
 * float32 addition (the drivers' own cur_time += dt).  It holds on every path that applies a grid update - mpm_grid_update,
 * mpm_substep (the dt actually used), mpm_run_fixed and the group drivers (whose fused carry-over applies the NEXT substep's
 * update and advances the clock then), mpm_mgsp_begin - exactly once per update.  The pose is computed on the host when the
 * update is enqueued and travels to the kernel by value.  Every rank of a group gets the same object and clock from its caller.
 * Neither the object nor its clock is part of a checkpoint: a restart installs the object again and calls
 * mpm_set_collision_clock with what mpm_get_collision_time returned when the checkpoint was saved.  HIP library only. */
int mpm_set_collision_clock(mpm_ctx* ctx, int running, float time);
int mpm_get_collision_time(mpm_ctx* ctx, float* time, int* running); /* either pointer may be NULL */

/* Extension (the reference knows level sets only): collision objects given in closed form.  They cost no device memory and no loads -
 * a level set keeps a float4 per node of the whole domain, 2 GiB at domain_bits 9 - and up to MPM_MAX_COLLISION_SHAPES of them can be
 * installed at once, beside the level-set object.  HIP library only.
 * Geometry.  A shape lives in the coordinates a level set's samples would be given in: a node at X is taken to the material point
 * x = R^T((X - shift) inv) scale + trans by the level set's own statements (the pose of mpm_set_collision_clock's comment), and the
 * shape answers with a signed distance sdis and a unit normal n:
 *   HALFSPACE  sdis = (x - a) . b^, n = b^                       (b^ = b / |b|, normalised on install)
 *   SPHERE     d = x - a, sdis = |d| - radius, n = d / |d|
 *   BOX        q = |x - a| - b per axis.  Inside (every q <= 0): sdis = max q, n = the axis of the largest q (ties: the lowest axis) with
 *              the sign of (x - a) on it (sign(0) = +).  Outside: sdis = |max(q, 0)|, n its gradient.
 *   CAPSULE    t = clamp((x - a) . (b - a) / |b - a|^2, 0, 1), d = x - (a + t (b - a)), sdis = |d| - radius, n = d / |d|
 * Where |d| = 0, n = 0 (nothing is divided by zero); the response then does what it does for a level set's zero gradient, SEPARATE's
 * early return included.  A node is touched when sdis <= 0; a NaN sdis touches nothing.  query_sdf's domain box does NOT apply: a
 * shape exists everywhere, in the wall zones too.  inside_out = 1: the solid is the complement (a container): sdis and n change sign.
 * Response.  From sdis <= 0 on, the level set's: object velocity in deformation space, STICKY / SLIP / SEPARATE, friction.
 * Several colliders.  Per cell with mass: walls and gravity; the level-set object, if installed; slots 0 .. 3 in order, each acting on
 * the velocity the previous one left.  With any collider installed mpm_grid_update reports the doubled |v|^2 of the final velocity.
 * Clock.  One per context, the level set's.  Every install of either kind sets it to obj->time, stopped; every removal stops it: install
 * all colliders, then call mpm_set_collision_clock once.  mpm_set_collision_clock / mpm_get_collision_time succeed when a level-set
 * object or any shape is installed.  Shapes are not part of a checkpoint; a checkpoint load leaves the installed ones in place. */
enum { MPM_SHAPE_HALFSPACE = 1, MPM_SHAPE_SPHERE = 2, MPM_SHAPE_BOX = 3, MPM_SHAPE_CAPSULE = 4 };
enum { MPM_MAX_COLLISION_SHAPES = 4 };
typedef struct mpm_collision_shape {
	int kind;
	int inside_out;	  /* 1: the solid is the complement (a container): sdis and n change sign */
	float a[3];		  /* HALFSPACE: a point of the plane; SPHERE / BOX: centre; CAPSULE: first end point */
	float b[3];		  /* HALFSPACE: outward normal (any length > 0; normalised on install); BOX: half extents (> 0); CAPSULE: second end point (!= a) */
	float radius;	  /* SPHERE, CAPSULE (> 0) */
	int reserved[5];
} mpm_collision_shape;
/* Install a shape in slot 0 .. 3 with the pose, motion and boundary fields of `obj`, or empty the slot (obj == NULL).  MPM_ERR_INVALID
 * (mpm_last_error names the field): slot outside 0..3, unknown kind, boundary type outside 0..2, radius or half extent <= 0 or not
 * finite, zero or non-finite normal, a capsule with a == b, a NaN anywhere in the shape. */
int mpm_set_collision_shape(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_collision_shape* shape);
/* Function-level entry point (as mpm_test_eig): on the device, for n arbitrary domain points xyz[n*3], the signed distance and normal the
 * grid kernels would use for this collider at `time` - out4[n*4] = {sdis, nx, ny, nz}.  dx is not used by the evaluation. */
int mpm_test_collision_shape(const mpm_collision_object* obj, const mpm_collision_shape* shape, float time, float dx, const float* xyz, size_t n, float* out4, int device);

/* Extension: a collision object given as a 2-D height table - terrain y = h(x, z) in material coordinates (up is material y; obj's rot_mat,
 * trans and trans_vel tilt and move it).  A 512 x 512 table is 1 MiB as heights and 4 MiB as installed, where the level set of the same
 * ground is a float4 per node of the whole domain.  HIP library only.
 * A heightfield occupies one of the four slots of mpm_set_collision_shape; either kind may sit in any slot, installing either kind over
 * the other replaces it (and frees the table), and mpm_set_collision_shape(ctx, slot, NULL, NULL) empties a heightfield slot too.  The
 * heightfield is reachable only through mpm_set_collision_heightfield: mpm_set_collision_shape goes on refusing every kind but 1 .. 4.
 * Everything the shapes' comment says about the pose, the response, the order of the colliders (field object, then slots 0 .. 3), the
 * doubled |v|^2 and the one clock holds word for word; like a shape, a heightfield is not part of a checkpoint.  The context owns the
 * table: it is freed on replace, on removal and in mpm_destroy.
 * Install (on the host).  From the heights H(i, k) one float4 {H, gx, gz, 0} per sample: gx = (H(i+1,k) - H(i-1,k)) / (2.f * spacing) in
 * the interior, (H(1,k) - H(0,k)) / spacing at i = 0, (H(nx-1,k) - H(nx-2,k)) / spacing at i = nx-1; gz the same along k.
 * Query at the material point x.  u = (x0 - origin0) / spacing, w = (x2 - origin1) / spacing.  Outside the footprint the collider touches
 * nothing, whatever inside_out says (sdis = NaN, n = 0): a point is outside unless 0 <= u <= (float) (nx-1) and 0 <= w <= (float) (nz-1); a
 * NaN is outside.  i = min((int) u, nx-2), k likewise; fu = u - (float) i, fw = w - (float) k; weights (1-fu)(1-fw), fu(1-fw), (1-fu)fw,
 * fu fw; each channel ((w00 t00 + w10 t10) + w01 t01) + w11 t11; len = sqrtf((gx gx + 1.f) + gz gz); n = (-gx, 1, -gz) / len;
 * sdis = (x1 - h) / len - the distance to the tangent plane, not a Euclidean distance: the response uses its sign only.  inside_out
 * changes the sign of sdis and n.  A node is touched when sdis <= 0. */
enum { MPM_HEIGHTFIELD_MAX_SAMPLES = 4096 }; /* per axis */
typedef struct mpm_heightfield {
	int nx, nz;		 /* samples along material x and z, each 2 .. MPM_HEIGHTFIELD_MAX_SAMPLES */
	float origin[2]; /* material (x, z) of sample (0, 0) */
	float spacing;	 /* > 0, finite: sample (i, k) sits at (origin[0] + i spacing, origin[1] + k spacing) */
	int inside_out;	 /* 1: the solid is ABOVE the surface (a ceiling) */
	int reserved[6];
} mpm_heightfield;
/* Install a heightfield in slot 0 .. 3 with the pose, motion and boundary fields of `obj`, or empty the slot (obj == NULL).
 * heights: nx * nz floats on the host, sample (i, k) at [i * nz + k]; copied during the call.  MPM_ERR_INVALID (mpm_last_error names the
 * field): slot outside 0..3, nx or nz outside 2..4096, spacing <= 0 or not finite, a NaN origin, a NULL hf or heights with a non-NULL obj,
 * boundary type outside 0..2, any height or derived table entry that is not finite.  A refused install leaves the slot's occupant in place. */
int mpm_set_collision_heightfield(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_heightfield* hf, const float* heights);
/* Function-level entry point (as mpm_test_collision_shape): out4[n*4] = {sdis, nx, ny, nz} at n arbitrary domain points xyz[n*3]. */
int mpm_test_collision_heightfield(const mpm_collision_object* obj, const mpm_heightfield* hf, const float* heights, float time, const float* xyz, size_t n, float* out4, int device);

/* Extension: the level-set collision object built on the device from a closed triangle mesh.  mpm_set_collision_mesh installs the object
 * mpm_set_collision_object installs - it replaces whichever of the two was there, sets the clock to obj->time, stopped, acts before slots
 * 0 .. 3 and is removed by mpm_set_collision_object(ctx, NULL, ...) - with the field computed by a kernel straight into the context's
 * float4 field: no N^3 host array and no staging.  HIP library only.
 * verts: nv x 3 floats in the coordinates a level set's samples are given in - node (i, j, k) samples the point ((float) i dx, (float) j dx,
 * (float) k dx); tris: nt x 3 vertex indices, counter-clockwise seen from outside.  Both are copied during the call.
 * Definition of the field (claymore_amd/csrc/mpm_collision_mesh.hpp; every float32 operation in the order written there, no contraction,
 * correctly rounded / and sqrtf):
 *   record of triangle t (host, float32): a, ab = b - a, ac = c - a, n^ = n / sqrtf(n . n) with n = ab x ac; for the sign only (float64,
 *     stored as float32, not bit-defined) a pseudonormal per edge - n^ of this triangle + n^ of the one across - and per corner - the sum
 *     over the triangles around the vertex of (interior angle at the vertex) x n^ (Baerentzen & Aanaes' angle-weighted normal);
 *   closest point c_t(p) by the Voronoi-region walk (Ericson's ClosestPtPointTriangle: d1 .. d6, va / vb / vc), which also yields the
 *     feature: corner a / b / c, edge ab / ac / bc, or face; q_t = |p - c_t|^2 as ((dx^2 + dy^2) + dz^2);
 *   nearest triangle T(p): the lowest t among the triangles with the smallest q_t (float32, strict < in index order);
 *   plane rule, where T's feature is the face or q_T < 2^-40 (a node on, or numerically on, the surface): sdis = (p - a) . n^ as
 *     ((x + y) + z), g = n^;
 *   radial rule elsewhere: d = sqrtf(q_T), s = +1 if (p - c_T) . m >= 0 else -1 with m the pseudonormal of T's feature, sdis = s d,
 *     g_k = s (p_k - c_k) / d;
 *   inside_out negates sdis and g.
 * The field covers every node of [0, N)^3 exactly: no band, no clamp.
 * Validation (host; MPM_ERR_INVALID, mpm_last_error names the reason; a refused install changes nothing: the installed object, if any,
 * stays): a NULL ctx / obj / verts / tris; boundary type outside 0..2; nt < 4, nt or nv above the limits; an index outside [0, nv); a
 * vertex that is not finite; a triangle whose n . n is zero or not finite in float32; a mesh that is not a closed, consistently oriented
 * manifold - every directed edge (u, v) must occur exactly once and its reverse (v, u) exactly once; a signed volume sum a . (b x c) / 6
 * (float64) <= 0 (flip the winding or use inside_out).  MPM_ERR_CAPACITY when the device cannot hold the new field (allocated while the
 * old one is still installed) or the triangle records, which live on the device for the duration of the call only; the context stays
 * usable and the old object stays installed. */
enum { MPM_MESH_MAX_TRIANGLES = 1 << 22, MPM_MESH_MAX_VERTICES = 1 << 22 };
typedef struct mpm_collision_mesh {
	int inside_out; /* 1: the solid is the complement (a container): sdis and g change sign */
	int reserved[7];
} mpm_collision_mesh;
int mpm_set_collision_mesh(mpm_ctx* ctx, const mpm_collision_object* obj, const mpm_collision_mesh* opt /* may be NULL */, const float* verts, size_t nv, const int32_t* tris, size_t nt);
/* The four words {sdis, gx, gy, gz} of the nodes of the box lo + [0, dims) of the installed level-set field, whichever call installed it,
 * bit for bit: node lo + (x, y, z) at out4[((x dims[1] + y) dims[2] + z) 4 ..].  MPM_ERR_INVALID without an installed level-set object, for
 * a NULL argument, a dims entry < 1 or a box that leaves [0, N)^3.  Reads only.  It is also how a built field is saved, to be installed
 * again through mpm_set_collision_object.  HIP library only. */
int mpm_get_collision_field(mpm_ctx* ctx, const int lo[3], const int dims[3], float* out4);

/* Extension: a collision object given as a local level-set box - a "volume": a dense table of {sdis, gx, gy, gz} samples with its own origin,
 * spacing and dimensions in material coordinates, in one of the four slots of mpm_set_collision_shape.  It is the heightfield's idea in three
 * dimensions: where the level-set object is one float4 per node of the whole domain (2 GiB at domain_bits 9), at the grid's resolution, once
 * per context, a volume of 96^3 samples is 14 MiB, its resolution is its own, and up to four of them - each with its own trans_vel, omega
 * and start pose, all on the context's one clock - act beside the level-set object.  HIP library only.
 * Any kind (shape, heightfield, volume) may sit in any slot; installing any kind over any other replaces it and frees its table, and
 * mpm_set_collision_shape(ctx, slot, NULL, NULL) empties a volume slot too.  A volume is reachable only through the two setters below:
 * mpm_set_collision_shape goes on refusing every kind but 1 .. 4.  Everything the shapes' comment says about the pose, the response, the
 * order of the colliders (field object, then slots 0 .. 3), the doubled |v|^2 and the one clock holds word for word; like a shape, a volume
 * is not part of a checkpoint.  The context owns the table: it is freed on replace, on removal and in mpm_destroy.
 * Table.  One float4 {sdis, gx, gy, gz} per sample, sample (i, j, k) at [(i * dims[1] + j) * dims[2] + k], at the material position
 * origin + ((float) i, (float) j, (float) k) * spacing (one multiplication, one addition per axis).
 * Query at the material point x (claymore_amd/csrc/mpm_collision_volume.hpp; float32, every operation in the order written, no contraction).
 * Per axis d: xl_d = x_d - origin_d, u_d = xl_d / spacing.  Outside the footprint the collider touches nothing, whatever inside_out says
 * (sdis = NaN, n = 0, nothing is loaded): a point is outside unless 0 <= u_d <= (float) (dims_d - 1) on all three axes; a NaN is outside.
 * Cell and weights are query_sdf's own statements on xl: cid_d = min((int) u_d, dims_d - 2), dis = xl_d - (float) cid_d * spacing,
 * w[d][0] = 1.f - dis / spacing, w[d][1] = dis / spacing.  The eight corners are summed in the level set's i, j, k loop order:
 * w = w[0][i] * w[1][j] * w[2][k]; sdis and the three gradient channels each start from 0.f and do += w * v.  nn = sqrtf(n0 n0 + n1 n1 +
 * n2 n2), n_d /= nn (a zero gradient gives what it gives in the level set); inside_out then negates sdis and n.  A node is touched when
 * sdis <= 0; a NaN touches nothing.  query_sdf's domain box does NOT apply: a volume exists wherever its footprint is.  With origin 0,
 * spacing dx and dims N these are the level-set kernel's statements on the same numbers. */
enum { MPM_VOLUME_MAX_SAMPLES = 1024 }; /* per axis */
typedef struct mpm_collision_volume {
	int dims[3];	 /* samples along material x, y, z: each 2 .. MPM_VOLUME_MAX_SAMPLES, product <= 2^27;
						all three 0 (mesh install only): size the box from the mesh, see below */
	float origin[3]; /* material position of sample (0, 0, 0) */
	float spacing;	 /* > 0, finite: sample (i, j, k) sits at origin + ((float) i, (float) j, (float) k) * spacing */
	int inside_out;	 /* 1: sdis and n change sign at the query */
	int pad;		 /* mesh install with dims 0: cells of margin around the mesh's bounding box; 0 means 2 */
	int reserved[7];
} mpm_collision_volume; /* 64 bytes */
/* Install a volume in slot 0 .. 3 with the pose, motion and boundary fields of `obj`, or empty the slot (obj == NULL).  field4:
 * dims[0] * dims[1] * dims[2] * 4 floats on the host, copied during the call.  MPM_ERR_INVALID (mpm_last_error starts "collision volume:"
 * and names the field): slot outside 0..3, a dim outside 2..1024 or a product above 2^27, zero dims, spacing <= 0 or not finite, a NaN
 * origin, pad < 0, boundary type outside 0..2, a NULL vol or field4 with a non-NULL obj, any sample that is not finite.  MPM_ERR_CAPACITY
 * when the device cannot hold the table, which is allocated beside the slot's old occupant.  A refused or failed install leaves the slot,
 * the clock and every other slot as they were. */
int mpm_set_collision_volume(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* field4);
/* The same with the table built on the device from a closed triangle mesh given in material coordinates (verts / tris and their validation:
 * mpm_set_collision_mesh's, every reason of which is reported behind "collision volume: ").  Sample (i, j, k) gets mpm_set_collision_mesh's
 * field definition - exact point-triangle distance by the Voronoi walk, the nearest triangle by strict < in index order, the plane or the
 * radial rule, the sign from the pseudonormals - evaluated at p_d = origin_d + (float) i_d * spacing, always outward-signed: vol->inside_out
 * acts at the query only.  With dims == {0, 0, 0} the host sizes the box from the mesh's bounding box [min, max] in float64 and stores the
 * origin as float32: origin_d = min_d - pad * spacing, dims_d = ceil((max_d - min_d) / spacing) + 2 * pad + 1 (pad 0 means 2; vol->origin is
 * not used); MPM_ERR_INVALID if that leaves the limits.  MPM_ERR_CAPACITY when the device cannot hold the table or the triangle records. */
int mpm_set_collision_volume_mesh(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* verts, size_t nv, const int32_t* tris, size_t nt);
/* The descriptor as installed (vol_out, may be NULL) and, unless out4 == NULL, the samples of the box lo + [0, dims) of the slot's table
 * bit for bit: sample lo + (x, y, z) at out4[((x dims[1] + y) dims[2] + z) 4 ..].  MPM_ERR_INVALID for a slot that holds no volume or a
 * box that leaves the table.  Reads only.  It is how a mesh-built volume is saved, to be installed again through mpm_set_collision_volume. */
int mpm_get_collision_volume(mpm_ctx* ctx, int slot, mpm_collision_volume* vol_out, const int lo[3], const int dims[3], float* out4);
/* Function-level entry point (as mpm_test_collision_heightfield): out4[n*4] = {sdis, nx, ny, nz} at n arbitrary domain points xyz[n*3]. */
int mpm_test_collision_volume(const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* field4, float time, const float* xyz, size_t n, float* out4, int device);

/* Extension: a model whose particles fill a closed triangle mesh, sampled on the device (claymore_amd/csrc/mpm_mesh_fill.hpp).  HIP library only.
 * verts / tris: as for mpm_set_collision_mesh, same coordinates, same validation.
 * Lattice (the reference's sample_uniform_box rule): node (i, j, k) carries 8 candidates at (((float) i + a 0.25f) dx, ((float) j + b 0.25f) dx,
 *   ((float) k + c 0.25f) dx), a, b, c in {-1, +1}; exact in float32.
 * Clip box: the nodes lo <= (i, j, k) < hi - opt->lo / opt->hi when opt->use_box, else [0, N)^3 -, cut per axis to
 *   floor(mn N) <= i < floor(mx N) + 2 with [mn, mx] the mesh's bounding box (float64 on the float32 vertices): the nodes that can carry a
 *   candidate inside the bounding box.  A particle in the wall zone is treated by mpm_initial_setup as one given to mpm_add_model.
 * Inside: inside(p) <=> sdis(p) < -margin, sdis the first word of mpm_set_collision_mesh's field definition evaluated at the candidate p
 *   with inside_out = 0 (nearest triangle, lowest index among equals; plane or radial rule); margin >= 0 keeps particles off the surface.
 *   |sdis| is bit-defined, its sign is the float64 pseudonormals' (not bit-defined where (p - c) . m is a rounding away from 0).
 * Order (it is the particle's id under mpm_track_particle_ids - the index in the array the model was added with): tiles of 4 x 4 x 4 nodes,
 *   aligned to the domain (tile = node >> 2), ascending with x slowest and z fastest; in a tile the nodes by (x 4 + y) 4 + z of their low
 *   bits; in a node a slowest, c fastest, -1 before +1.
 * MPM_ERR_INVALID: what mpm_set_collision_mesh refuses in a mesh; a margin that is negative or not finite; a lo / hi entry outside [0, N].
 * hi <= lo on an axis, or a mesh that holds no candidate, gives 0 points (an empty model is legal).  MPM_ERR_CAPACITY when the device
 * cannot hold the work buffers (64 B + 4 B per tile of the clipped range, the triangle records) or the positions.  A refused call changes
 * nothing, the context stays usable; every work buffer is released before the call returns. */
typedef struct mpm_mesh_fill {
	float margin;
	int lo[3], hi[3];
	int use_box; /* 0: the whole domain */
	int reserved[8];
} mpm_mesh_fill;
/* The points only, without a context (N = 2^domain_bits, dx = 1 / N, domain_bits 4 .. 10): count, then fetch - mpm_grid_isosurface's
 * protocol.  xyz NULL: *n receives the count.  Else *n is the capacity of xyz (points) on entry and the count on return; MPM_ERR_CAPACITY
 * with the true count in *n, and nothing written, when it is too small. */
int mpm_sample_mesh(int domain_bits, const float* verts, size_t nv, const int32_t* tris, size_t nt, const mpm_mesh_fill* opt /* may be NULL */, float* xyz, size_t* n, int device);
/* mpm_add_model with the positions sampled straight into the model's own device array (no host array, no staging); its preconditions
 * (before mpm_initial_setup, at most 8 models, the material range).  *n_out (may be NULL): the particle count. */
int mpm_add_model_mesh(mpm_ctx* ctx, int material, const mpm_material_params* params, const float* verts, size_t nv, const int32_t* tris, size_t nt,
					   const mpm_mesh_fill* opt /* may be NULL */, const float v0[3], int* model_id, size_t* n_out);
/* Function-level entry point: a timed mpm_sample_mesh that keeps the points on the device.  out8 = {points, tiles of the clipped range,
 * tiles decided from their centre, classify ms, scan ms, emit ms, 0, 0}. */
int mpm_test_mesh_fill(int domain_bits, const float* verts, size_t nv, const int32_t* tris, size_t nt, const mpm_mesh_fill* opt /* may be NULL */, double* out8, int device);

/* Extension (the reference starts every particle at rest in its material, all with one velocity): per-particle initial conditions - the
 * inverse of the readouts above.  Set-up only: a model given none of this is set up exactly as mpm_add_model's.  HIP library only.
 * mpm_add_model_particles is mpm_add_model with up to four arrays in the order of xyz, copied to the device during the call, checked there
 * and released when mpm_initial_setup returns:
 *   velocity  v_p in world units (NULL: v0 for every particle);
 *   affine9   the APIC matrix C_p, column-major exactly as mpm_retrieve_velocity returns it: affine9[9*i + 3*c + r] = C_rc (NULL: 0).
 *             The set-up P2G gives node i the momentum m w_ip (v_p + C_p (x_i - x_p)), x_i - x_p in world units;
 *   state9    the inverse of mpm_retrieve_state (NULL: the stress-free state).  Solids with state_kind MPM_STATE_B: the symmetric b = F F^T as
 *             mpm_retrieve_state returns it, the sign of entry 0 marking a reflected F; the entries [0] [4] [8] and [1] [2] [5] are read and
 *             stored verbatim, so readout -> re-seed -> readout is bit for bit.  Solids with MPM_STATE_F: F in the layout of mpm_test_stress's
 *             input (column-major); the library forms b = F F^T in float32 and sets the mark where det F < 0.  MPM_J_FLUID: state9[9*i] is J
 *             with MPM_STATE_B, and J = det of the 3 x 3 with MPM_STATE_F;
 *   logjp     log Jp (MPM_SAND / MPM_NACC only, ignored for the other materials; NULL: params->log_jp0).
 * init == NULL is mpm_add_model.
 * mpm_set_model_velocity_field gives a model that has been added, by any of the three calls - mpm_add_model_mesh's models included, whose
 * positions never reach the host -, the linear field v_p = v0 + G (x_p - pivot), C_p = G, evaluated in the set-up kernel (grad9 column-major:
 * grad9[3*c + r] = G_rc; NULL pointers read as zeros).  It replaces the model's v0; APIC with quadratic B-splines carries a linear field
 * exactly, so mpm_retrieve_velocity returns the field and G right after set-up (a spinning or shearing body).
 * Errors: MPM_ERR_INVALID, mpm_last_error says which, and a refused call changes nothing - after mpm_initial_setup; a reserved word that is
 * not 0; an unknown state_kind; a value that is not finite in any array or in the field; |b00|, b11, b22 or J not strictly positive; a
 * velocity field on a model that was added with a velocity or affine9 array; a model number that does not exist.  MPM_ERR_CAPACITY when the
 * device cannot hold the arrays. */
typedef struct mpm_particle_init {
	const float* velocity; /* n*3, world units.  NULL: v0 for every particle */
	const float* affine9;  /* n*9, C_p, column-major exactly as mpm_retrieve_velocity returns it
							  (affine9[9*i + 3*c + r] = C_rc).  NULL: 0 */
	const float* state9;   /* n*9.  NULL: stress-free (mpm_add_model's state) */
	const float* logjp;	   /* n, SAND / NACC only.  NULL: params->log_jp0 */
	int state_kind;		   /* what state9 holds for FC / SAND / NACC: MPM_STATE_B or MPM_STATE_F */
	int reserved[3];	   /* must be 0 */
} mpm_particle_init;
int mpm_add_model_particles(mpm_ctx* ctx, int material, const mpm_material_params* params, const float* xyz, size_t n, const float v0[3],
							const mpm_particle_init* init /* NULL == mpm_add_model */, int* model_id);
int mpm_set_model_velocity_field(mpm_ctx* ctx, int model, const float v0[3], const float grad9[9] /* column-major */, const float pivot[3]);

/* Extension (the reference's scenes hold the particles they start with): add n particles to model `model` of a context that has been set up -
 * an inflow.  HIP library only, single contexts only.  xyz, v0 and the arrays of `init` mean exactly what mpm_add_model_particles says (NULL
 * arrays: v0, C_p = 0, the stress-free state, params->log_jp0), are checked on the device the same way, and the model's material and
 * parameters are reused.  An empty model, and a context whose models are all empty, can be emitted into.
 * When: at a substep boundary with the grid holding momenta - mpm_retrieve_velocity's state, which mpm_initial_setup, mpm_substep,
 * mpm_run_fixed and mpm_checkpoint_load leave.
 * What it is: a re-lay, O(all particles) per call like a capacity growth or a checkpoint load, not a change of the substep loop (DESIGN.md
 * 3.8).  Afterwards
 *   - every old particle's position and stored state (b with its mark, or J; log Jp) and, in a tracked context, its id have the bits they
 *     had; the new particles carry the given state bit for bit; the particle order of the readouts is unspecified as always;
 *   - a grid node that no new particle's 27-node stencil reaches has the bits it had (its block may have a new number); a node that is
 *     reached holds the old value plus m w for the mass and m w (v_p + C_p (x_i - x_p)) for the momentum of every new particle - the
 *     set-up P2G of mpm_add_model_particles, without a stress term, as at set-up;
 *   - the model's particle count and mpm_get_counts grow by n; the cumulative lost / dropped / discarded counters are untouched;
 *   - in a tracked context the new particles have the ids old n .. old n + n - 1 in input order (n: everything the model was ever given);
 *     *first_id (may be NULL) receives old n in an untracked context too;
 *   - the next rebuild is not offered the still path; the collision clock, colliders, rigid bodies, the load gauge and the timers are untouched.
 * Capacities grow by the usual policy (mpm_config.grow; mpm_get_capacity's growth_events counts it).  Transient device memory: 56 B per
 * particle of the context (52 B untracked) plus the old grid, released before return.
 * Checkpoints: one saved after emissions carries the grown n; it loads into a context whose models were added with that many particles
 * (any positions: they only size it), ids through mpm_particle_ids_load as usual.
 * Errors - a refused call changes nothing, every readout, checkpoint and later substep is bit for bit that of a context that never saw it:
 * MPM_ERR_NOT_READY before mpm_initial_setup.  MPM_ERR_INVALID for a bad model; a NULL xyz with n > 0; a reserved word that is not 0; an
 * unknown state_kind; a value that is not finite; a state that is not strictly positive; a position set-up would count as outside the
 * domain; a grid that holds velocities (between mpm_grid_update and mpm_rebuild_partition); a context that belongs or belonged to a group or
 * has been through the halo tagging; a tracked context whose ids are not valid.  MPM_ERR_CAPACITY for a block that would hold more than
 * max_ppc * 64 particles of the model (whatever drop_overflow says, as at set-up), with grow = 0 for block or bin capacities that do not
 * suffice, and when the device cannot hold the staging arrays.  n == 0 is MPM_OK and changes nothing.
 * Not offered: groups and MGSP ranks, an incremental emission inside the rebuild.  (Removal: mpm_remove_particles below.) */
int mpm_emit_particles(mpm_ctx* ctx, int model, const float* xyz, size_t n, const float v0[3], const mpm_particle_init* init /* may be NULL */,
					   int32_t* first_id /* may be NULL */);

/* Extension: take particles out of a context that has been set up - a sink, emission's mirror image.  HIP library only, single contexts only.
 * Which particles: a live particle of a selected model (model >= 0: that one; -1: all) goes when the signed distance of any region at its
 * position is <= 0, or when its id is in `ids`.  The regions are mpm_collision_shape's four kinds in domain coordinates, without a pose: the
 * point that is tested is the particle's float32 world position, as the readouts return it, and the distance is the very function the
 * colliders evaluate.  They pass the checks of mpm_set_collision_shape (a half-space's normal is normalised the same way); inside_out selects
 * the complement; a NaN distance selects nothing.  `ids` (tracked contexts, model >= 0) names particles of that model; an id that names no live
 * particle is ignored and not counted, duplicates are fine.  mpm_count_particles_in is the predicate alone: out[m] = how many particles of
 * model m the regions select; it writes nothing.
 * When: mpm_emit_particles' preconditions - after set-up, at a substep boundary with the grid holding momenta, a single context that never
 * belonged to a group, ids valid if tracked.
 * What it is: a re-lay, O(all particles) like an emission, not a change of the substep loop.  A removed particle's share of
 * the grid momentum cannot be subtracted exactly (v_p and C_p exist only in the registers of the substep kernels) - and need not be: what the
 * next substep reads off the grid is the node velocity p / m, and the next P2G rewrites mass and momentum.  So the removal keeps every node's
 * velocity and gives it the mass of the particles that remain.  Afterwards
 *   - every survivor's position and stored state (b with its mark, or J; log Jp) and, in a tracked context, its id have the bits they had;
 *   - mpm_get_counts shrinks by removed[m]; the model's n - everything it was ever given - stays: a later emission continues its ids from n
 *     and a removed id never returns; the cumulative lost / dropped / discarded counters are untouched; a checkpoint saved afterwards loads
 *     like one saved after particles were lost;
 *   - a grid node that no removed particle's 27-node stencil reaches has the bits it had (its block may have a new number).  A reached node
 *     with old mass m_old > 0: with m' the set-up rasteriser's mass of all surviving particles of all models at that node, m' == 0 leaves +0 in
 *     all four channels, else the mass is m' and each momentum p_old * r, r = m' / m_old (one float32 division).  A reached node whose old mass
 *     is not > 0 keeps its bits.  A block of the old grid that the survivors' partition does not hold is dropped;
 *   - out->removed[m]: particles taken out of model m; out->mass and out->momentum: mpm_grid_totals before the call minus after it;
 *     out->relaid = 1, and the next rebuild is not offered the still path.  Capacities neither shrink nor grow.  A model may become empty,
 *     and so may every model of the context.
 * Nothing selected: MPM_OK with relaid = 0.  The call has launched its count pass alone, the context is untouched bit for bit and the still
 * path stays on offer - which is what makes a sink that is polled every few substeps affordable.
 * removed_xyz (3 per particle) / removed_ids / removed_model (any may be NULL; `capacity` particles each) receive the removed particles in an
 * unspecified order, the three arrays row by row alike; the id is -1 in an untracked context.
 * Errors - a refused call changes nothing: mpm_emit_particles' list (MPM_ERR_NOT_READY before set-up; MPM_ERR_INVALID for a bad model, a
 * non-zero reserved word, a grid that holds velocities, a group or halo-tagged context, ids that are not valid), MPM_ERR_INVALID for an invalid
 * region or nregions > 8, for `ids` with model < 0 or in an untracked context, for an id outside 0 .. n - 1; MPM_ERR_CAPACITY when `capacity`
 * is smaller than the number selected (out->removed then holds the true counts) or the device cannot hold the staging arrays (emission's
 * 56 B per surviving particle, the old grid, 1 KiB per neighbour block for m', 20 B per removed particle).  MPM_ERR_INTERNAL if a dropped block
 * held mass at a node no removed particle reaches.
 * Not offered: groups and MGSP ranks, the oracle, a removal inside the substep. */
enum { MPM_MAX_SINK_REGIONS = 8 };
typedef struct mpm_removal {
	const mpm_collision_shape* regions; /* nregions of them, 0..8 */
	int nregions;
	const int32_t* ids; /* nids of them; NULL with nids == 0 */
	size_t nids;
	float* removed_xyz;	/* capacity * 3, may be NULL */
	int32_t* removed_ids;	/* capacity, may be NULL */
	int32_t* removed_model; /* capacity, may be NULL */
	size_t capacity;
	int reserved[4]; /* must be 0 */
} mpm_removal;
typedef struct mpm_removal_result {
	int64_t removed[8];
	double mass;
	double momentum[3];
	int relaid;
	int reserved[3];
} mpm_removal_result;
int mpm_count_particles_in(mpm_ctx* ctx, int model /* -1: all */, const mpm_collision_shape* regions, int nregions, int64_t out[8]);
int mpm_remove_particles(mpm_ctx* ctx, int model /* -1: all */, const mpm_removal* what, mpm_removal_result* out /* may be NULL */);

/* Current capacities and the number of times check_capacity() (gmpm_simulator.cuh:283-300) has grown them: blocks
 * (exterior count limit), bins per model (bin_capacity[8]).  HIP library only. */
int mpm_get_capacity(mpm_ctx* ctx, int64_t* block_capacity, int64_t* bin_capacity, int* growth_events);
int mpm_get_timers(mpm_ctx* ctx, mpm_timers* t);
/* What the reference loses silently, counted since initial_setup (as of the last completed rebuild): particles that left
 * the domain or the block neighbourhood (add_advection finds no block, particle_buffer.cuh:105-113) and P2G contributions
 * discarded because a particle moved more than one cell in a substep (mgmpm_kernels.cuh:877-885, a CFL violation).
 * A run that conserves mass has both at zero; bench.py and the full-size tests assert that.  HIP library only. */
typedef struct mpm_diagnostics {
	int64_t lost_particles;
	int64_t discarded_p2g;
	int overflow_flags; /* bit 0: block capacity, bit 1: particles per block (MPM_ERR_CAPACITY, unless bit 1 with drop_overflow) */
	int dropped_particles; /* cumulative; only with mpm_config.drop_overflow */
	int reserved[3];
	int still_rebuilds; /* rebuilds since initial_setup that kept the partition (mpm_config.still_rebuild), as of the last synchronisation */
} mpm_diagnostics;
int mpm_get_diagnostics(mpm_ctx* ctx, mpm_diagnostics* d);
/* Sum over the current grid of {mass, momentum x, y, z} (the reference's sum_grid_mass debug kernel,
 * mgmpm_kernels.cuh:1034-1037, extended to momentum); valid between rebuild and the next grid update. */
int mpm_grid_totals(mpm_ctx* ctx, double out[4]);
/* Table consistency of the current partition (the reference's check_table debug kernel, mgmpm_kernels.cuh:1022-1032): the number of blocks i
 * with query(active_keys[i]) != i plus the number of table entries that belong to no block; 0 = consistent; negative = error. */
int mpm_check_table(mpm_ctx* ctx);
/* Dense dump of the current grid for parity tests: for every neighbor block, key (3 ints) and 256 floats
 * {mass[64], mvx[64], mvy[64], mvz[64]} (grid_buffer.cuh:12-14 layout). *nblocks in = capacity, out = count. */
int mpm_dump_grid(mpm_ctx* ctx, int* keys, float* blocks, size_t* nblocks);
/* Debug read-out of the per-block look-up rows of `model` in the current numbering (HIP library only; read-only, synchronises the compute
 * stream like mpm_dump_grid): for every particle block 64 ints - [0, 27) the first source bin per direction, [27, 54) the destination block
 * numbers, [54, 62) the grid block numbers, 62 / 63 unused.  *nblocks in = capacity in blocks, out = the particle block count. */
int mpm_dump_block_rows(mpm_ctx* ctx, int model, int32_t* rows, size_t* nblocks);
/* Extension (the reference has no Eulerian output): what the grid holds between two substeps - the mass m_i and momentum p_i of the last
 * P2G - read out by position instead of by particle.  N = 2^domain_bits nodes per axis; node (i, j, k) sits at
 * (i, j, k) dx.  A node holds a value only if it lies in [0, N)^3 AND its block (i >> 2, j >> 2, k >> 2) is in the current partition's table
 * AND that block's number is below neighbor_blocks (the numbering mpm_dump_grid reports): the exterior blocks, numbers neighbor_blocks ..
 * exterior_blocks - 1, are known to the table but have no grid rows.  Every other node reads as +0.
 * mpm_sample_grid: out4[4 q .. 4 q + 3] = sum_i W_i(x_q) {m_i, p_i x, y, z} for each of n world-space points xyz[3 q ..], over the 27-node
 *   quadratic B-spline stencil formed exactly as G2P forms it: p_d = x_d * 2^domain_bits in one float32 multiply, base_d = lround(p_d) - 1
 *   (ties away from zero), weights of p_d - base_d, W = w0[i] w1[j] w2[k] at node base + (i, j, k).  A point with any p_d not finite, < 0
 *   or >= N gets four zeros.  n = 0 is legal and launches nothing.  The outputs are raw sums in mass and momentum units: / dx^3 gives
 *   densities, and sum W p / sum W m the mass-weighted velocity - deliberately NOT the sum W (p_i / m_i) of mpm_retrieve_velocity, which
 *   at a point without particles is biased toward zero by the empty nodes of the stencil.
 * mpm_grid_volume: out as [4][dims[0]][dims[1]][dims[2]] float32 (channel-major: mass, px, py, pz; z fastest).  Output cell (X, Y, Z)
 *   covers the stride^3 nodes origin + stride (X, Y, Z) + [0, stride)^3.  stride 1: the node's four words, copied bit for bit.  stride 2
 *   or 4: acc = +0.0f, acc += value over the covered nodes in float32, x slowest and z fastest - a sum, so totals are conserved.  origin
 *   may be negative and the box may leave the domain (those nodes read zero).  MPM_ERR_INVALID for a stride other than 1, 2, 4, a dims
 *   entry < 1 or 16 dims[0] dims[1] dims[2] overflowing size_t; MPM_ERR_CAPACITY when the device cannot hold the box (the context stays usable).
 * mpm_grid_box_totals: out = {sum m, sum px, sum py, sum pz, sum_{m > 0} |p|^2 / (2 m)} over the nodes of the half-open node box [lo, hi),
 *   clipped to the domain; float64 sums of the float32 node values, in an unspecified order (the last bits may differ between calls).  An
 *   empty box gives five zeros.  For [0, N)^3 the first four are mpm_grid_totals' up to summation order.
 * Preconditions and errors: those of mpm_retrieve_velocity - MPM_ERR_NOT_READY before mpm_initial_setup; MPM_ERR_INVALID for a NULL array,
 * for a grid that holds velocities (between mpm_grid_update and the next mpm_rebuild_partition) and, permanently, for a context that has
 * ever joined an mpm_group or been through the halo tagging: there is no group form of these calls.  They read only: no state, checkpoint
 * or later substep changes.  HIP library only. */
int mpm_sample_grid(mpm_ctx* ctx, const float* xyz, size_t n, float* out4);
int mpm_grid_volume(mpm_ctx* ctx, const int origin[3], const int dims[3], int stride, float* out);
int mpm_grid_box_totals(mpm_ctx* ctx, const int lo[3], const int hi[3], double out[5]);
/* Extension: the iso-surface of the mass grid - a watertight triangle soup, by marching tetrahedra over the valued blocks only.
 * Field: f(i, j, k) is the mass word of node (i, j, k) as mpm_grid_volume at stride 1 reads it: the valued nodes are those above, every
 *   other node - exterior or absent blocks, the nodes -1 and N just outside the domain - reads +0.  A node is INSIDE iff f > iso_mass (a
 *   NaN is outside).  iso_mass must be finite and > 0 (else MPM_ERR_INVALID): the field is 0 outside a bounded set, so the surface of the
 *   whole grid is closed.  Density is f / dx^3.
 * Cells: cell (i, j, k), i, j, k in [-1, N - 1], has the eight corner nodes (i, j, k) + {0, 1}^3.  lo and hi both NULL: every cell.  Both
 *   given: the cells with lo <= (i, j, k) < hi only - a half-open CELL box that may leave the domain; the surface is open where the box
 *   cuts it.  Exactly one of them NULL: MPM_ERR_INVALID.
 * Tetrahedra: the six Kuhn tetrahedra of the cell, one per permutation (a, b, c) of the axes, with the corners c0 = (0, 0, 0), c1 = c0 +
 *   e_a, c2 = c1 + e_b, c3 = (1, 1, 1).  All share the main diagonal; the decomposition is the same in every cell, so neighbouring cells
 *   agree on the diagonals of their common face.
 * Vertices: an edge (A, B) of a tetrahedron, A the corner that is componentwise <= B (B - A is in {0, 1}^3), carries a vertex iff exactly
 *   one end is inside.  t = (iso_mass - f(A)) / (f(B) - f(A)): two float32 subtractions and one correctly rounded float32 division, in
 *   [0, 1] whenever both masses are finite.  In node units the vertex is (float) A_d + t on the axes with B_d - A_d = 1 (one float32 add)
 *   and (float) A_d on the others; the world position is that times dx (exact).  The value depends on the edge's two nodes only, so
 *   triangles that share an edge get BIT-IDENTICAL vertices: a caller welds on the position bits.
 * Triangles: one inside corner I and outside corners O0 < O1 < O2 (in the tetrahedron's corner order): P(I, O0) P(I, O1) P(I, O2); three
 *   inside: the mirror case P(I0, O) P(I1, O) P(I2, O); two inside I0 < I1, outside O0 < O1: the quad P(I0, O0) P(I0, O1) P(I1, O1)
 *   P(I1, O0) split along P(I0, O0) - P(I1, O1).  Winding: the normal (v1 - v0) x (v2 - v0) points from the inside corners to the outside
 *   corners, decided from the CORNER coordinates - the sign of det[O0 - I, O1 - I, O2 - I], for the quad the same test on the edge
 *   midpoints - never from interpolated positions: the order above is kept or reversed.  Degenerate triangles (t rounded to 0 or 1) so
 *   keep a defined winding; they are kept, not filtered.  Which vertex of a triangle comes first, and the order of the triangles, are
 *   unspecified.
 * Output: tri_xyz[9 q ..] the three world-space vertices of triangle q; tri_vel[9 q ..] (may be NULL) per vertex (p(A) + t (p(B) - p(A)))
 *   / iso_mass per momentum channel - the mass-weighted velocity there, the interpolated mass being iso_mass - in float32, in any
 *   association.  *n in: the capacity in triangles; out: the number of triangles the surface HAS.  tri_xyz NULL: count only (tri_vel
 *   must be NULL too), nothing but the count is computed.  A count above the capacity: MPM_ERR_CAPACITY, *n the true count, the buffers
 *   hold `capacity` triangles of the surface, unspecified which; the context stays usable and the caller retries (mpm_halo_keys'
 *   protocol).  MPM_ERR_CAPACITY also when the device cannot hold the staging buffer of 72 (with tri_vel 144) bytes a triangle (*n is
 *   then left as it was).
 * Non-finite masses: inside or outside by the comparison above, so the count is always defined; the positions and velocities of the
 *   vertices on an edge with a non-finite end are unspecified.
 * Preconditions and errors: those of mpm_grid_volume - MPM_ERR_NOT_READY before mpm_initial_setup; MPM_ERR_INVALID for a NULL n, for a
 * grid that holds velocities and, permanently, for a context that has ever joined an mpm_group or been through the halo tagging.  Reads
 * only: no state, checkpoint or later substep changes.  HIP library only. */
int mpm_grid_isosurface(mpm_ctx* ctx, float iso_mass, const int lo[3], const int hi[3], float* tri_xyz, float* tri_vel, size_t* n);
/* Collider loads (an extension, the reference has none): what the NEXT grid update with this dt will do to every massed
 * node, collider by collider - read off grid[0] while it holds the mass and momentum of the last P2G, with the colliders as installed and their
 * poses at the clock's current time.  Nothing is written: not the grid, not the clock.
 * Rows: 0 the level-set object, 1 .. 4 the slots 0 .. 3, 5 the domain walls (gravity belongs to no row).  Per node and row, in the grid update's
 *   own float32 statements: dv = v_after - v_before (the wall row: 0 - p / m on each axis a wall zeroes); the node is touched where a component of
 *   dv is non-zero or NaN.  j = (double) m * (double) dv is the impulse on the material, -j the load on the collider, r x (-j) its torque with
 *   r = (double) ((float) node * dx) - pivot.
 * mpm_collider_loads: out[row] = {touched nodes, Jx, Jy, Jz, Lx, Ly, Lz, touched mass}, J = sum(-j), L = sum r x (-j); force and torque over the
 *   step are J / dt and L / dt.  Pivots: a row's default is its collider's shift at the clock's time (trans + trans_vel T), the wall row's the
 *   origin; opt (may be NULL) replaces those whose has_pivot is non-zero.  float64 sums in a fixed order without atomics: the same state
 *   gives the same bits on every call.  Non-finite grids get no special treatment.
 * mpm_collider_contacts: one record per touched (node, row): node_row4 int32 {i, j, k, row}, rec8 float32 {m, dv[3], v_after[3], 0}, in no
 *   particular order.  mpm_grid_isosurface's protocol: *n in: the capacity in records (node_row4 NULL: count only); out: the number there ARE;
 *   a count above the capacity is MPM_ERR_CAPACITY with the true count.
 * mpm_load_gauge: on != 0 zeroes the accumulators and from then on every stand-alone grid update (mpm_grid_update, mpm_substep, mpm_run_fixed,
 *   which then no longer fuses the next update into the carry-over: same results, bit for bit) first adds its loads, its dt and 1 to them, on
 *   the stream, without a host synchronisation; opt as above, kept and applied at every update (a default pivot follows its collider).  on == 0 releases it.  Off (the default) nothing is
 *   allocated or launched.  Not part of a checkpoint: mpm_checkpoint_load zeroes the accumulators.
 * mpm_load_gauge_read: the accumulated rows, the float64 sum of the dts and the number of updates (any pointer may be NULL); reset != 0 zeroes them.
 * Errors: MPM_ERR_NOT_READY before mpm_initial_setup; MPM_ERR_INVALID for a NULL out / n, dt <= 0 or NaN, a grid that holds velocities, a context
 *   that has ever joined an mpm_group or been through the halo tagging, mpm_load_gauge_read with the gauge off.  HIP library only. */
#define MPM_LOAD_ROWS 6
typedef struct mpm_load_options {
	int has_pivot[MPM_LOAD_ROWS];
	float pivot[MPM_LOAD_ROWS][3];
} mpm_load_options;
int mpm_collider_loads(mpm_ctx* ctx, float dt, const mpm_load_options* opt, double out[MPM_LOAD_ROWS][8]);
int mpm_collider_contacts(mpm_ctx* ctx, float dt, int32_t* node_row4, float* rec8, size_t* n);
int mpm_load_gauge(mpm_ctx* ctx, int on, const mpm_load_options* opt);
int mpm_load_gauge_read(mpm_ctx* ctx, double out[MPM_LOAD_ROWS][8], double* elapsed, int* updates, int reset);
/* Rigid bodies (an extension; INTEGRATION.md section 5, claymore_amd/csrc/mpm_rigid_body.hpp): a BODY is a slot collider whose pose and velocity
 * are state on the device instead of functions of the collision clock.  Every applied grid update treats it as prescribed at its present
 * (x, q, v, omega): the material's nodes take the response, and the body afterwards takes the equal and opposite impulse - J and L of its load
 * row above, L about x - so what grid and body exchange is conserved to the last bit per update.
 * Eligible: slots 0 .. 3 holding a SPHERE, a BOX, a CAPSULE or a volume.  MPM_ERR_INVALID (mpm_last_error names the reason) for an empty slot, a
 *   HALFSPACE or a heightfield (unbounded); obj.scale != 1 or obj.dsdt != 0; an obj.rot_mat that is not a rotation (|R^T R - I| entries above
 *   1e-5, det < 0); mass <= 0 or not finite; an inertia that is not symmetric positive definite; a NaN anywhere; non-zero reserved words; a
 *   context that belongs or belonged to a group or has been through the halo tagging.  A group refuses to adopt a context that has a body.  The
 *   level-set object (row 0) cannot be a body.  A refused call changes nothing.
 * Start: where the collider stands at the moment of the call.  q0 from obj.rot_mat; the slot's object is re-pivoted to the centre of mass
 *   (internal trans := com, x0 = trans + R0 (com - trans) in float64: every node's material point is what it was, up to float32 rounding, exactly
 *   so when com == obj.trans and rot_mat is the identity); v0 = obj.trans_vel; omega0 = obj.omega read as a TRUE angular velocity (world; not
 *   the plus-sign cross product of the prescribed colliders); l0 = R Ib R^T omega0.  A body ignores the collision clock: it advances with every
 *   applied grid update, whether the clock runs or not.
 * The step, h = (double) dt, in float64 with + - x / and sqrt alone:
 *   v <- v + (J + h force) / mass (+ (double) gravity * h on y with the gravity flag), locked components 0, x <- x + h v;
 *   l <- l + L + h torque, omega = R(q) Ib^-1 R(q)^T l, locked components 0 (then l <- R Ib R^T omega);
 *   q <- (q + h/2 (0, omega) (x) q) / |...|: the axis and the norm are exact, the angle falls short by (h |omega|)^3 / 12 per step.
 *   lock bits 0 .. 2: world translation x, y, z; 3 .. 5: rotation about world x, y, z.  A non-finite J, L or state: MPM_ERR_NONFINITE at the
 *   next synchronisation.
 * The coupling is explicit: stable while the mass of the touched nodes stays below the body's; max_mass_ratio is the largest ratio seen.
 *   Bodies do not collide with each other, with prescribed colliders or with the domain walls.  With a body installed mpm_run_fixed keeps the
 *   grid update a kernel of its own (as with the load gauge); mpm_collider_loads' default pivot of a body row is its x at the time of the call.
 * mpm_set_collider_body on a slot that already holds a body gives it new constants: q, v, omega, the counters and the last impulses keep their float64
 *   words, x moves by R(q) (com_new - com_old) so that no node's material point moves, l = R Ib_new R^T omega.
 * mpm_set_collider_body: body NULL makes the slot prescribed again, at rest at the pose it has reached.  Installing any collider over the slot,
 *   or emptying it, removes the body.  mpm_get_collider_body: either output may be NULL; MPM_ERR_INVALID for a slot without a body.
 * mpm_set_collider_body_state: a restart; a NULL keeps that part; the orientation is normalised, l follows from omega.  Bodies, like colliders,
 *   are not part of a checkpoint: a load leaves them as they are.
 * mpm_shape_mass_properties, mpm_mesh_mass_properties: mass, inertia and com of a homogeneous solid of `density`, in the coordinates the shape
 *   or the mesh is given in (gravity = 1, lock = 0, force = torque = 0); host only, no context: the closed forms of sphere, box and capsule,
 *   float64 polyhedral integrals under mpm_set_collision_mesh's validation.  HIP library only. */
typedef struct mpm_rigid_body {
	float mass;
	float inertia[6]; /* xx yy zz xy xz yz, body frame, about com */
	float com[3];
	int gravity;
	int lock;
	float force[3];
	float torque[3];
	int reserved[8]; /* must be 0 */
} mpm_rigid_body;
typedef struct mpm_rigid_body_state {
	double position[3], orientation[4] /* w x y z */, velocity[3], omega[3], angular_momentum[3], last_impulse[3], last_angular_impulse[3], last_touched_mass, max_mass_ratio;
	int64_t last_touched_nodes, updates;
} mpm_rigid_body_state;
int mpm_set_collider_body(mpm_ctx* ctx, int slot, const mpm_rigid_body* body);
int mpm_get_collider_body(mpm_ctx* ctx, int slot, mpm_rigid_body* body_out, mpm_rigid_body_state* state_out);
int mpm_set_collider_body_state(mpm_ctx* ctx, int slot, const double position[3], const double orientation[4], const double velocity[3], const double omega[3]);
int mpm_shape_mass_properties(const mpm_collision_shape* shape, float density, mpm_rigid_body* out);
int mpm_mesh_mass_properties(const float* verts, size_t nv, const int32_t* tris, size_t nt, float density, mpm_rigid_body* out);

/* Extension (the reference knows one scalar gravity on y): force fields on the grid - a tilted gravity, wind, a stirrer, an attractor, damping.
 * Up to MPM_MAX_FORCE_FIELDS of them, in slots 0..3, installed, replaced and removed at any substep boundary.  Every applied grid update then
 * applies them to the {mass m, momentum p} of every grid node with mass, BEFORE walls, gravity and colliders, slots in order, each on the
 * momentum the previous one left; the mass is never written.  X is the node position the collider slots see.  HIP library only.
 * Region and weight w.  `region` is an mpm_collision_shape in domain coordinates, without pose or clock (as mpm_remove_particles' regions;
 *   inside_out is honoured); region.kind 0: w = 1 everywhere.  feather == 0: w = sdis <= 0 ? 1 : 0.  feather > 0: w = sdis < 0 ?
 *   min(1, -sdis / feather) : 0.  A NaN sdis gives 0.  A node with w == 0 is skipped by that slot: its words keep their bits.
 * Kinds (float32, no contraction, + - * / sqrtf only; INTEGRATION.md section 5 has the order of every operation):
 *   UNIFORM  a = vec.
 *   POINT    r = centre - X, d2 = r.r + soft^2, d = sqrt(d2); a = strength r / d (falloff 0), strength r / d2 (1), strength r / (d2 d) (2);
 *            d == 0 gives a = 0; a negative strength repels.
 *   VORTEX   the axis n^ = vec / |vec| (normalised on install) runs through centre: r = X - centre, rp = r - (r.n^) n^,
 *            a = swirl (n^ x rp) - pull rp + lift n^.
 *   these three: p += m a (w dt).
 *   DRAG     toward the velocity vec at the rate strength (wind; damping with vec = 0), implicit Euler of dv/dt = -w strength (v - vec):
 *            s = w strength dt, p = (p + s m vec) / (1 + s).
 * With a field installed mpm_run_fixed keeps every grid update a launch of its own (the fields' pass runs ahead of it); a context without
 * one allocates and launches nothing for this.  mpm_collider_loads / mpm_collider_contacts and the load gauge see the forced momenta; fields
 * belong to no load row, as gravity belongs to none.  Fields do not act on rigid bodies, are not part of a checkpoint (a load leaves the
 * installed ones in place, the parameter hash does not know them) and are not offered in multi-GPU groups and MGSP ranks. */
enum { MPM_FORCE_UNIFORM = 1, MPM_FORCE_POINT, MPM_FORCE_VORTEX, MPM_FORCE_DRAG };
enum { MPM_MAX_FORCE_FIELDS = 4 };
typedef struct mpm_force_field {
	int kind;
	int falloff;	 /* POINT: 0, 1 or 2 (others: 0) */
	float vec[3];	 /* UNIFORM: acceleration; VORTEX: axis (any length > 0; normalised on install); DRAG: target velocity */
	float centre[3]; /* POINT, VORTEX */
	float strength;	 /* POINT: pull (negative: repels); DRAG: rate (>= 0) */
	float swirl, pull, lift; /* VORTEX */
	float soft;		 /* POINT: softening length (>= 0) */
	float feather;	 /* width of the region's soft edge (>= 0) */
	mpm_collision_shape region; /* kind 0: everywhere */
	int reserved[6]; /* must be 0 */
} mpm_force_field;
/* Install a field in slot 0..3 or empty the slot (f == NULL).  MPM_ERR_INVALID (mpm_last_error names the field; a refused call changes
 * nothing): slot outside 0..3, unknown kind or falloff, any non-finite number, a zero axis, strength < 0 for DRAG, soft < 0 or feather < 0, a
 * region mpm_set_collision_shape would refuse, a reserved word that is not 0; a context that belongs, or belonged, to a group or an MGSP
 * rank (and mpm_group_create* refuse a context with a field installed). */
int mpm_set_force_field(mpm_ctx* ctx, int slot, const mpm_force_field* f);
/* The field as installed (unit axis, unit region normal); kind 0: the slot is empty. */
int mpm_get_force_field(mpm_ctx* ctx, int slot, mpm_force_field* out);
/* Function-level entry point (as mpm_test_collision_shape): the fields' statements for one node, on the device, at n arbitrary points
 * xyz[n*3] with given {m, p} mp4[n*4] -> out4[n*4]; fields[i] sits in slot i (kind 0: empty), n_fields 0..4.  The fields are validated as
 * mpm_set_force_field validates them before the device is touched.  dx is not used by the evaluation. */
int mpm_test_force_field(const mpm_force_field* fields, int n_fields, float dt, float dx, const float* xyz, const float* mp4, size_t n, float* out4, int device);
/* How the library was built: "claymore_hip <abi> experiment=<none | list of -D switches>".  A product library reports
 * experiment=none (claymore_amd/csrc/mpm_device_math.hpp: the switches that change what the kernels compute only exist under
 * -DMPM_EXPERIMENT); tests/test_abi.py asserts it for the shipped library.  Needs no device. */
const char* mpm_build_info(void);
/* G2P2G kernel time of the last call on the compute stream's own clock (mpm_run_fixed: of the last substep, from the phase stamps its kernels
 * write; MPM_PHASE_TIMERS=events in the environment at mpm_create keeps HIP events for every substep). */
int mpm_last_g2p2g_ms(mpm_ctx* ctx, float* ms);
/* The launch-size rule of the rebuild's three kernels that only look and leave on a still substep (mpm_run_fixed): workgroups of its prepare launch and
 * of its two registration launches, 0 = the full size, given the still streak at the last read-back, whether the still path is on, the particle block
 * count and the setting MPM_STILL_LAUNCH=auto|full|thin:N would give (null = unset = auto, which leaves the registrations at their full size; thin:N
 * is for tests and A/B).  Needs no device. */
int mpm_still_launch_sizes(const char* setting, int streak, int still_on, int particle_blocks, int* prepare_workgroups, int* register_workgroups);

/* ---- function-level entry points used by the parity tests (device versions of the per-particle math) ---- */
/* What the constitutive models take from math::svd (Library/MnBase/Math/Matrix/svd.cuh:27-1123; they need U and the singular
 * values only, V cancels): the eigen-decomposition F F^T = U diag(lam) U^T, lam_k = sigma_k^2, U a rotation, columns in no
 * particular order.  F[n*9] column-major -> out[n*12] = U(9) lam(3). */
int mpm_test_eig(const float* F, size_t n, float* out12, int device);
/* compute_stress<M> (Projects/GMPM/constitutive_models.cuh) on deformation gradients F[n*9]: out19 = b'(9) PF(9) logjp'(1), b' the
 * left Cauchy-Green tensor F' F'^T of the model's (possibly projected) F' - what a particle of this engine stores. */
int mpm_test_stress(int material, const mpm_material_params* p, const float* F, const float* logjp, size_t n, float* out19, int device);

/* ---- multi-GPU (MGSP static particle partition, Projects/MGSP/mgsp_benchmark.cuh:661-776) ----
 * One context per rank/GPU owns a fixed particle subset; grids of different ranks overlap only in blocks touched by
 * particles of both.  All buffers named dev_* are DEVICE pointers supplied by the caller (e.g. torch tensors) so that
 * the transport (RCCL all-gather / all-to-all over xGMI) stays outside this library.  The exchange kernels run on the
 * context's comm stream, ordered against the compute stream with events inside the library. */
/* Copy this rank's neighbor-block keys (ivec3, count = neighbor_blocks) into dev_keys: the payload of the all-gather
 * that replaces the pairwise cudaMemcpyAsync of mgsp_benchmark.cuh:681-686.  At most capacity_blocks keys are copied;
 * *count always receives the true number, so a caller with a too small buffer can retry. */
int mpm_halo_keys(mpm_ctx* ctx, int* dev_keys, int capacity_blocks, int* count);
/* reset_overlap_marks / reset counts (mgsp_benchmark.cuh:690-692). */
int mpm_halo_tag_begin(mpm_ctx* ctx);
/* mark_overlapping_blocks (halo_kernels.cuh:21-35): dev_peer_keys = npeer_keys ivec3 of peer `peer` (0..31); marks this
 * rank's neighbor blocks that the peer also owns and builds the send list for that peer. */
int mpm_halo_tag_peer(mpm_ctx* ctx, int peer, const int* dev_peer_keys, int npeer_keys);
/* collect_blockids_for_halo_reduction (halo_kernels.cuh:37-62): split the particle blocks into halo / interior lists and
 * read the per-peer send counts back.  send_counts (host, 32 ints, may be NULL) receives them. */
int mpm_halo_tag_end(mpm_ctx* ctx, int* halo_particle_blocks, int* send_counts);
/* Phases of a multi-GPU substep (mgsp_benchmark.cuh:421-465): clears + g2p2g on the halo list, then on the interior list. */
int mpm_g2p2g_halo(mpm_ctx* ctx, float dt, float next_dt);
int mpm_g2p2g_interior(mpm_ctx* ctx, float dt, float next_dt);
/* collect_grid_blocks (halo_kernels.cuh:64-80): gather the blocks shared with `peer` from grid `gid` (1 = this step's
 * P2G target, 0 = current grid, used once after initial_setup) into dev_keys (n*3 ints) / dev_blocks (n*256 floats). */
int mpm_halo_collect(mpm_ctx* ctx, int peer, int gid, int* dev_keys, float* dev_blocks, int capacity_blocks, int* nsend);
/* reduce_grid_blocks (halo_kernels.cuh:82-97): add nrecv received blocks into grid `gid` (hardware f32 atomics). */
int mpm_halo_reduce(mpm_ctx* ctx, int gid, const int* dev_keys, const float* dev_blocks, int nrecv);
/* Debug read-out of the last tagging (mpm_halo_tag_end or mpm_mgsp_end), in the style of mpm_check_table / mpm_dump_grid; host arrays,
 * each may be NULL: overlap[neighbor_blocks] = the marks, bit p set iff the block is shared with peer p (bit 31 is the sign bit);
 * halo_list[*n_halo] = the halo particle blocks in no particular order (capacity: particle_blocks); inner_flags[particle_blocks] = 1 for
 * an interior block, 0 for a halo block.  Block numbers index mpm_halo_keys' list.  MPM_ERR_INVALID before the first tagging.  Read-only
 * (it waits for the context's streams).  Not to be called inside an open fused substep: between mpm_mgsp_rebuild_export and mpm_mgsp_end
 * the marks already belong to the new partition while the counts that size the copies are still the old one's.  HIP library only. */
int mpm_halo_dump(mpm_ctx* ctx, int* overlap, int* halo_list, int* n_halo, int* inner_flags);
/* ---- fused multi-GPU substep: the same phases with ONE host synchronisation per substep ----
 * (the phase-by-phase calls above synchronise once each, like the reference's issue()/sync() barriers,
 * mgsp_benchmark.cuh:336-356; at 5 M particles per GPU that costs more than the kernels.)
 *   mpm_mgsp_begin        : grid update (no read-back) + clears + G2P2G on the halo list
 *   mpm_halo_collect xN, all-to-all-v, mpm_g2p2g_interior, mpm_halo_reduce xN      (as above)
 *   mpm_mgsp_rebuild_export: partition rebuild launches + padded key export for the all-gather: dev_keys holds
 *                            pad_rows rows of 3 ints, row 0 = {neighbor-block count, 0, 0}, rows 1.. = keys
 *   all-gather of the padded key lists (caller)
 *   mpm_mgsp_tag          : overlap marks / send lists / halo split from the gathered lists (world*pad_rows rows),
 *                            all sizes read on the device
 *   mpm_mgsp_end          : the one synchronisation: counts, send counts (32), halo block count, max |v|^2 of this
 *                            step's grid update; rolls the double buffers.  *max_peer_rows = largest key-list length
 *                            (+1) any rank exported: if it exceeds pad_rows the caller re-tags with a larger pad. */
int mpm_mgsp_begin(mpm_ctx* ctx, float dt, float next_dt);
int mpm_mgsp_rebuild_export(mpm_ctx* ctx, int* dev_keys, int pad_rows);
int mpm_mgsp_tag(mpm_ctx* ctx, const int* dev_all_keys, int pad_rows, int world, int rank);
int mpm_mgsp_end(mpm_ctx* ctx, int* send_counts, int* halo_particle_blocks, int* max_peer_rows, float* max_vel_sqr);

/* HIP stream handles (as void*) so that the caller can order collectives against the engine. */
int mpm_streams(mpm_ctx* ctx, void** compute_stream, void** comm_stream);
int mpm_sync(mpm_ctx* ctx);

/* ---- MGSP group driver: the multi-GPU substep loop in C++ on RCCL (MgspBenchmark::main_loop, mgsp_benchmark.cuh:361-559;
 * worker threads issue()/sync() :309-356; tagging :661-720; halo exchange :723-776, halo_buffer.cuh:54-59).  One group
 * handle per rank, each on its own context.  Transport of mpm_group_create: RCCL (ncclAllGather for the block keys,
 * ncclGroup{ncclSend, ncclRecv} for the symmetric halo exchange on the context's comm stream, ncclAllReduce(max) for dt);
 * the caller only has to carry the 128-byte unique id from rank 0 to the other ranks (MPI, a file, torch.distributed ...).
 * mpm_group_create_local builds `world` handles in ONE process (contexts may share a device) on device-to-device copies:
 * single-GPU boxes, tests, and hosts that drive all GPUs from worker threads; its calls must be made concurrently, one
 * thread per rank.  The environment variable MPM_RCCL_LIBRARY names the collective library to load instead of the system's
 * librccl.so (a differently built RCCL; the tests' in-process double, tests/rccl_double/).  HIP library only. */
typedef struct mpm_group mpm_group;
int mpm_group_unique_id(void* id128);
int mpm_group_create(mpm_ctx* ctx, int rank, int world, const void* id128, mpm_group** out);
int mpm_group_create_local(mpm_ctx* const* ctxs, int world, mpm_group** out /* [world] */);
void mpm_group_destroy(mpm_group* g);
const char* mpm_group_last_error(const mpm_group* g);
/* The transport the group ended up with: "rccl", "peer-direct" (one process, several devices, hipMemcpyPeerAsync behind the peer's events:
 * the reference's own mechanism, halo_buffer.cuh:54-59) or "device-copy" (contexts of one device, or a pair of devices without peer access:
 * synchronous copies behind host barriers).  A caller that asked for peer-direct reports the fall-back with it. */
const char* mpm_group_transport(const mpm_group* g);
/* initial_setup of every rank + first tagging + one exchange that sums the rasterised grids (mgsp_benchmark.cuh:561-659). */
int mpm_group_initial_setup(mpm_group* g);
/* Restart (row f4 for the multi-GPU loop; the reference has none): after EVERY rank has loaded its own checkpoint with
 * mpm_checkpoint_load (taken after a call of this driver returned), rebuild what a checkpoint does not carry - padded key length,
 * overlap marks, halo / interior lists, per-peer send lists.  Collective: every rank calls it. */
int mpm_group_resume(mpm_group* g);
/* One substep, one host synchronisation; *max_vel_sqr = this rank's max |v|^2 (not reduced over ranks). */
int mpm_group_substep(mpm_group* g, float dt, float next_dt, float* max_vel_sqr);
int mpm_group_run_fixed(mpm_group* g, int nsteps, float dt);
/* compute_dt of the MGSP project (Projects/MGSP/utility_funcs.hpp:32-55): CFL 0.3 and the 0.51 frame-remainder rule. */
float mpm_group_compute_dt(const mpm_group* g, float max_vel, float cur_time, float next_time, float dt_default);
/* main_loop with adaptive dt from the maximum grid velocity over all ranks (:410-418); on_frame may be NULL. */
int mpm_group_main_loop(mpm_group* g, int frames, int fps, float dt_default, void (*on_frame)(int frame, void* user), void* user, int* steps_out);
int mpm_group_stats(const mpm_group* g, int* send_counts32, int* halo_particle_blocks, float* g2p2g_ms_avg);
/* Readout of a group (extension).  At the return of a group call that completed (mpm_group_initial_setup,
 * _resume, _substep, _run_fixed) and inside mpm_group_main_loop's on_frame, every rank's grid holds the mass and momentum summed over the
 * ranks on every node its particles reach, and the readout of mpm_retrieve_velocity is evaluated on it.
 * mpm_group_retrieve_velocity: this rank's particles of `model` (positions, v_p, C_p as mpm_retrieve_velocity; affine9 may be NULL).
 *   Per rank, NOT collective: it may be called from on_frame.
 * mpm_group_particle_momentum: the five totals of mpm_particle_momentum over the particles of ALL ranks (model = -1: all models).
 *   Collective: every rank calls it; every rank gets the same bits (the ranks' float64 sums gathered and added in rank order).  A rank
 *   that cannot read out makes the call fail on every rank.
 * Errors: MPM_ERR_NOT_READY before set-up; MPM_ERR_INVALID for a bad model or NULL array, after a group call that failed, and after a
 * phase-level call on the context (mpm_grid_update, mpm_g2p2g*, mpm_rebuild_partition, mpm_mgsp_*, mpm_halo_*, mpm_checkpoint_load ...)
 * until the next group call completes; MPM_ERR_CAPACITY when *n is too small.  A readout error does not break the group. */
int mpm_group_retrieve_velocity(mpm_group* g, int model, float* xyz, float* vel, float* affine9, size_t* n);
int mpm_group_particle_momentum(mpm_group* g, int model, double out[5]);

#ifdef __cplusplus
}
#endif
#endif
