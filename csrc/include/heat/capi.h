/* C ABI of libheat.so — consumed by the Python package (ctypes) and usable
 * from any language.  All functions return 0 on success and -1 on error;
 * heat_last_error() then returns a thread-local message.
 *
 * Two layers:
 *   heat_solver_*  the full per-rank engine (fields, passes, exchange, graphs)
 *   heat_op_*      single kernels on caller-owned device buffers, for tests
 *                  and for composing custom schedules (stream = hipStream_t).
 */
#ifndef HEAT_CAPI_H
#define HEAT_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HEAT_ABI_VERSION 9

typedef struct heat_params {
  int64_t nx, ny;
  float cx, cy;
  int32_t converge, check_interval;
  double eps;
  int32_t init;      /* heat::InitMode */
  uint64_t seed;
  int32_t backend;   /* 0 cpu, 1 hip */
  int32_t kernel;    /* 0 auto, 1 naive, 2 tb */
  int32_t tb_depth;
  int32_t threads;
  int32_t decomp;    /* 0 auto(2-D), 1 rows, 2 grid2d */
  int32_t px, py;
  int32_t use_graph, overlap;
  int32_t compat;    /* 0 none, 1 mpi, 2 cuda */
  int32_t device;
  int32_t schedule;    /* 0 auto, 1 sync, 2 overlap (exchange-first), 3 pipeline */
  int32_t halo_passes; /* sync schedule: passes per exchange (0 = auto) */
  int32_t numerics;    /* 0 fp32 (canonical FMA), 1 mpi (reference MPI double arithmetic) */
  int32_t phase_timing;/* 1: per-phase times in heat_run_stats (disables graphs) */
  int32_t insulated;   /* insulated (zero-flux) plate edges: 1 north, 2 south, 4 west, 8 east */
  int32_t periodic;    /* periodic (wrap-around) axes: 1 x (north-south joined), 2 y (west-east) */
} heat_params;

/* Options added after heat_params was frozen (heat_solver_create_ex).  `size` is
 * sizeof(heat_params_ext) as the caller knows it: fields beyond it take their
 * defaults, so later options need no new entry point. */
typedef struct heat_params_ext {
  int32_t size;
  int32_t source;  /* 1: the run has a per-cell heat source (heat_solver_set_source):
                      u' = stencil(u) + q, the src kernel, a third field */
} heat_params_ext;

/* Transport selection for heat_solver_create. */
typedef struct heat_comm {
  int32_t kind;          /* 0 local, 1 rccl, 2 tcp, 3 callback, 4 loopback (ctx = hub) */
  int32_t rank, world;
  int32_t device;        /* rccl: HIP device */
  uint8_t unique_id[128];/* rccl: ncclUniqueId from heat_rccl_unique_id on rank 0 */
  const char* addr;      /* tcp: rank-0 address */
  int32_t port;          /* tcp: rank-0 port */
  /* callback transport */
  void* ctx;
  int (*sendrecv)(void* ctx, const void* msgs /* heat_msg[n] */, int n);
  int (*allreduce)(void* ctx, void* buf, int count, int dtype);
  int (*barrier)(void* ctx);
} heat_comm;

typedef struct heat_run_stats {
  int64_t steps_done, total_steps;
  int32_t converged;
  int64_t converged_at;
  float last_resid;
  double seconds;
  int64_t passes, exchanges, checks;
  double t_exchange, t_compute, t_reduce; /* seconds per phase (phase_timing) */
  int64_t resident_passes;                /* passes run inside resident-tile launches */
  int64_t resident_giveups;               /* 1: a resident launch gave up (HEAT_TB_RES_GIVEUP=defer) */
  int64_t chained_passes;                 /* passes run inside chained level-split launches */
} heat_run_stats;

typedef struct heat_block_info {
  int32_t rank, world, px, py, cx, cy;
  int64_t ox, oy, lx, ly;
  int32_t nbr[4]; /* north, south, west, east; -1 = none */
  int64_t pitch, rows;
  int32_t hx, hy, halo, tb_depth;
  int64_t bytes_per_field;
  int32_t schedule; /* effective heat::Schedule (1 sync, 2 overlap, 3 pipeline) */
  int32_t insulated; /* the run's insulated plate edges (heat_params.insulated) */
  int32_t periodic;  /* the run's periodic axes (heat_params.periodic) */
  int32_t pad_;
} heat_block_info;

typedef struct heat_checksum {
  uint64_t hash;
  double sum, min, max;
  int64_t count;
} heat_checksum;

typedef struct heat_solver heat_solver;
typedef struct heat_transport heat_transport;

typedef struct heat_transport_info {
  int32_t nranks;      /* rccl: ncclCommCount; else the world size */
  int32_t device;      /* rccl: ncclCommCuDevice; else -1 */
  int32_t user_rank;   /* rccl: ncclCommUserRank; else the rank */
  char bus_id[32];     /* PCI bus id of `device` ("" if unknown) */
  char name[16];       /* transport name */
} heat_transport_info;

const char* heat_last_error(void);
int heat_abi_version(void);
const char* heat_build_info(void);

int heat_rccl_unique_id(uint8_t out[128]);
int heat_device_count(int* n);

int heat_solver_create(const heat_params* p, const heat_comm* c, heat_solver** out);
/* A transport (e.g. one RCCL communicator) that several solvers use in turn:
 * each solver keeps a reference, so destroying the handle early is safe. */
int heat_transport_create(const heat_comm* c, heat_transport** out);
int heat_transport_destroy(heat_transport* t);
int heat_transport_info_get(heat_transport* t, heat_transport_info* out);
int heat_solver_create_shared(const heat_params* p, heat_transport* t, heat_solver** out);
/* The same with the extended options (ext may be NULL: the defaults). */
int heat_solver_create_ex(const heat_params* p, const heat_params_ext* ext, const heat_comm* c,
                          heat_solver** out);
int heat_solver_create_shared_ex(const heat_params* p, const heat_params_ext* ext,
                                 heat_transport* t, heat_solver** out);
int heat_solver_destroy(heat_solver* s);
int heat_solver_run(heat_solver* s, int64_t steps, heat_run_stats* out);
/* Asynchronous run (plain GPU runs): enqueue the steps and return; the next
   heat_solver_run (steps 0: just complete) waits for them and checks errors. */
int heat_solver_enqueue(heat_solver* s, int64_t steps, heat_run_stats* out);
/* RCCL on one rank: self send/recv (eager or hipGraph-captured) + all-reduce. */
int heat_rccl_self_test(int device, int64_t bytes, int graph, int iters, double* gbps);
/* RCCL abort while another thread issues calls on the communicator (one-rank
   communicators, `rounds` rounds); *calls = calls completed before the aborts. */
int heat_rccl_abort_race_test(int device, int rounds, int* calls);
/* Loopback transport: ranks are threads of this process sharing one hub. */
int heat_loopback_hub_create(int world, void** out);
int heat_loopback_hub_destroy(void* hub);
/* A rank of the hub failed: peers blocked in an exchange or collective throw. */
int heat_loopback_hub_fail(void* hub);
/* Transport of a single-process multi-rank run (ranks = threads, rank r on
   devices[r]): requested "auto" | "rccl" | "loopback"; *kind = 1 (rccl: every
   rank has a GPU of its own) or 4 (loopback: ranks share a device).  The rule
   of heat::choose_group_transport, shared by `heat --gpus N` and
   parallel.group.run_group. */
int heat_group_transport(const char* requested, int world, const int32_t* devices, int32_t* kind);
/* Give up this rank: abort its transport (ncclCommAbort) so peers stop
   waiting; a wait of the solver on another thread throws.  Thread-safe. */
int heat_solver_abort(heat_solver* s);
/* Seconds per grouped halo exchange of `depth` rows/columns on this rank
   (device time over `iters` exchanges) and its largest message; collective. */
int heat_solver_time_exchange(heat_solver* s, int depth, int iters, double* seconds,
                              int64_t* max_bytes);
/* 1 if the automatic TB variant at `depth` takes a residual at any inner step
   (checks ride inside full-depth passes), else 0. */
int heat_tb_mid_residual(int depth);
int heat_solver_reset(heat_solver* s);
int heat_solver_info(heat_solver* s, heat_block_info* out);
int heat_solver_step(heat_solver* s, int64_t* out);
int heat_solver_copy_owned(heat_solver* s, float* host, int64_t host_pitch);
int heat_solver_load_owned(heat_solver* s, const float* host, int64_t host_pitch, int64_t step);
/* rank 0: host must hold nx*ny floats; other ranks: host may be NULL */
int heat_solver_gather(heat_solver* s, float* host);
int heat_solver_checksum(heat_solver* s, heat_checksum* out);
/* Coarse view of the current state: per fx x fy coarse cell the fp64 sum, the
   min and the max, into host arrays of CR*CC (heat_coarse_dims) on every rank.
   Collective; changes nothing of the run. */
int heat_solver_coarse(heat_solver* s, int64_t fx, int64_t fy, double* sum, float* min,
                       float* max);
/* Fill the whole plate from the cr x cc host grid S by refinement (factors fx, fy;
   order 0 piecewise constant, 1 cell-centred bilinear; an axis wraps where the run
   is periodic), each rank its own block where it lives, then continue at `step`
   like heat_solver_load_owned.  Not collective; every rank passes the same S.
   heat_solver_reset still returns to the formula initial condition. */
int heat_solver_refine(heat_solver* s, const float* S, int64_t cr, int64_t cc, int64_t fx,
                       int64_t fy, int order, int64_t step);
/* Heat source of a solver created with heat_params_ext.source: q = the refinement
   of the cr x cc host grid S (factors, order, limits and wrapping of
   heat_solver_refine), filled into the rank's block and its ghost ring without
   communication; S == NULL clears it (all +0).  Not part of the state: reset,
   refine, load, scatter and read_bin keep it, checkpoints do not store it.  Not
   collective; every rank passes the same S.  Fails on a solver without the option. */
int heat_solver_set_source(heat_solver* s, const float* S, int64_t cr, int64_t cc, int64_t fx,
                           int64_t fy, int order);
/* Tests: the source field's rows and columns [-halo, l + halo) of this rank. */
int heat_solver_copy_source(heat_solver* s, float* host, int64_t host_pitch, int halo);
/* rank 0: full holds nx*ny floats (row-major); other ranks: full may be NULL */
int heat_solver_scatter(heat_solver* s, const float* full, int64_t step);
int heat_solver_write_bin(heat_solver* s, const char* path);
int heat_solver_read_bin(heat_solver* s, const char* path);
int heat_solver_barrier(heat_solver* s);
int heat_solver_current_ptr(heat_solver* s, void** ptr);

/* host utilities */
int heat_write_dat(const char* path, int64_t nx, int64_t ny, const float* grid);
int heat_format_6_1f(float v, char* out, int cap);
int heat_dims_create(int nnodes, int ndims, int* dims);
int heat_block_span(int64_t n, int parts, int index, int64_t* offset, int64_t* size);
int heat_init_value(int mode, int64_t ix, int64_t iy, int64_t nx, int64_t ny, uint64_t seed,
                    float* out);
int heat_cpu_step(const float* src, float* dst, int64_t pitch, int64_t gx0, int64_t gy0, int64_t nx,
                  int64_t ny, float cx, float cy, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                  float* resid /* may be NULL */);

/* device ops (pointers are device pointers to local cell (0,0); stream is a hipStream_t) */
int heat_op_naive_step(const float* src, float* dst, int64_t pitch, int64_t gx0, int64_t gy0,
                       int64_t nx, int64_t ny, float cx, float cy, int64_t r0, int64_t r1,
                       int64_t c0, int64_t c1, unsigned* resid, void* stream);
int heat_op_lds_step(const float* src, float* dst, int64_t pitch, int64_t gx0, int64_t gy0,
                     int64_t nx, int64_t ny, float cx, float cy, int64_t r0, int64_t r1,
                     int64_t c0, int64_t c1, unsigned* resid, void* stream, int numerics);
int heat_op_mfma_step(const float* src, float* dst, int64_t pitch, int64_t gx0, int64_t gy0,
                      int64_t nx, int64_t ny, float cx, float cy, int64_t r0, int64_t r1,
                      int64_t c0, int64_t c1, unsigned* resid, void* stream);
/* One step with a per-cell source q (the layout of src and dst):
   u' = stencil(u) + q over the box, fp32 numerics; `gate` (may be NULL): a device
   word, non-zero = the launch writes nothing.  Device kernel and host twin. */
int heat_op_source_step(const float* src, float* dst, const float* q, int64_t pitch, int64_t gx0,
                        int64_t gy0, int64_t nx, int64_t ny, float cx, float cy, int64_t r0,
                        int64_t r1, int64_t c0, int64_t c1, unsigned* resid, void* stream,
                        const unsigned* gate);
int heat_cpu_source_step(const float* src, float* dst, const float* q, int64_t pitch, int64_t gx0,
                         int64_t gy0, int64_t nx, int64_t ny, float cx, float cy, int64_t r0,
                         int64_t r1, int64_t c0, int64_t c1, float* resid /* may be NULL */);
/* The launch plan heat_op_source_step takes (heat::gpu::source_plan) with the
   planner's constants, a cap on the waves of a launch (0 = default) for tests, and
   the switch of non-temporal q loads and dst stores (1 on, 0 off, -1 = the default:
   on when a step sweeps more than 256 MiB).  Both knobs are for tests and
   tools/source_bench.py only: they are process-global and change every launch
   of every solver in the process. */
typedef struct heat_source_plan {
  int64_t strips, chunks, units;
  int32_t chunk_rows, waves, align, vector_rows;
  int32_t strip_cols, max_chunk_rows, min_chunk_rows, waves_per_cu; /* constants */
} heat_source_plan;
int heat_op_source_plan(const float* src, const float* dst, const float* q, int64_t pitch,
                        int64_t r0, int64_t r1, int64_t c0, int64_t c1, heat_source_plan* out);
int heat_op_source_max_waves(int waves);
int heat_op_source_nontemporal(int mode);
/* k fused source steps in one launch (heat::gpu::source_tb_step), 2 <= k <= 8:
   dst on the box is what k calls of heat_op_source_step give, call j over the box
   grown by k-1-j and clipped to the plate; resid: the last level's.  Device only. */
int heat_op_source_tb_step(const float* src, float* dst, const float* q, int64_t pitch,
                           int64_t gx0, int64_t gy0, int64_t nx, int64_t ny, float cx, float cy,
                           int64_t r0, int64_t r1, int64_t c0, int64_t c1, int k, unsigned* resid,
                           void* stream, const unsigned* gate);
/* Its launch plan (heat::gpu::source_tb_plan) with the planner's constants, and a
   cap on the waves of a launch (0 = default; process-global, for tests).  With a
   cap set the plan needs no device: it depends on the addresses' alignment only. */
typedef struct heat_source_tb_plan_t {
  int64_t strips, chunks, units;
  int32_t chunk_rows, waves, align, vector_rows, overlap, strip_stride;
  int32_t strip_cols, max_chunk_rows, min_chunk_rows, waves_per_cu, max_depth; /* constants */
  int32_t pad_;
} heat_source_tb_plan_t;
int heat_source_tb_plan(const float* src, const float* dst, const float* q, int64_t pitch,
                        int64_t r0, int64_t r1, int64_t c0, int64_t c1, int k,
                        heat_source_tb_plan_t* out);
int heat_source_tb_set_max_waves(int waves);
/* Fused launches this process has enqueued so far (solvers' and heat_op_source_tb_step's). */
int64_t heat_source_tb_launches(void);
// Diagnostics: per-wave start/end clock stamps of subsequent TB launches
// (4 u64 per wave: start, end at 100 MHz, block, strip<<32|chunk); null = off.
int heat_op_tb_stamps(void* buf, int64_t waves);
int heat_op_tb_step(const float* src, float* dst, int64_t pitch, int64_t gx0, int64_t gy0,
                    int64_t nx, int64_t ny, float cx, float cy, const int64_t* boxes /* nbox*4 */,
                    int nbox, int depth, unsigned* resid, void* stream, int waves_target,
                    int variant /* -1 default; heat::gpu::tbv flags */,
                    int res_level /* residual step 1..depth, 0 = depth */);
/* TB launch-planner knobs (heat::gpu::TbTuning); weights: up to 4 age-group shares;
   tile_rows / tile_waves: rows per wave / waves per workgroup of tile launches
   (0 = planner); tile_xl: tile lane shifts 0 DPP, 1 ds_bpermute, 2 mixed (-1 = default);
   nt: level-split rows non-temporal 1 / plain 0 (-1 = by the bytes a pass sweeps). */
typedef struct heat_tb_tuning {
  int32_t variant, rounds, min_len, waves;
  double edge_frac;
  int32_t n_weights, tile_rows;
  double weights[4];
  int32_t tile_waves, tile_xl;
  int32_t nt, pad_;
} heat_tb_tuning;
int heat_tb_get_tuning(heat_tb_tuning* out);
int heat_tb_set_tuning(const heat_tb_tuning* in);
int heat_op_init(float* origin, int64_t lx, int64_t ly, int halo, int64_t gx0, int64_t gy0,
                 int64_t nx, int64_t ny, int mode, uint64_t seed, void* stream);
int heat_op_pack(const float* origin, int64_t pitch, int64_t r0, int64_t r1, int64_t c0,
                 int64_t c1, float* buf, void* stream);
int heat_op_unpack(const float* buf, float* origin, int64_t pitch, int64_t r0, int64_t r1,
                   int64_t c0, int64_t c1, void* stream);
int heat_op_residual(const float* a, const float* b, int64_t pitch, int64_t r0, int64_t r1,
                     int64_t c0, int64_t c1, unsigned* resid, void* stream);
/* n <= 8 boxes (r0, r1, c0, c1 each) <-> their contiguous device buffers in one
   launch (the packing / unpacking of a halo exchange); empty boxes are skipped. */
int heat_op_copy_boxes(float* origin, int64_t pitch, const int64_t* boxes /* n*4 */,
                       float* const* bufs /* n device pointers */, int n, int to_buf, void* stream);
/* The device-side convergence decision (heat::gpu::judge_check): `gate` is an
   8-word device record {stop, reason, stop_check, checks, last_bits, pad[3]};
   check i of the n is the max over s < slots of resid[s * stride + i]. */
int heat_op_judge(unsigned* resid, void* gate, double eps, int mpi_compat, int n, int slots,
                  int stride, void* stream);
/* Checksum of an lx x ly block whose cell (0,0) is cell (ox, oy) of a plate with
   ny columns: the device kernel (waits for it), and its host twin on host memory. */
int heat_op_checksum(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                     int64_t oy, int64_t ny, heat_checksum* out, void* stream);
int heat_cpu_checksum(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                      int64_t oy, int64_t ny, heat_checksum* out);
/* Coarse view: CR = ceil(nx/fx), CC = ceil(ny/fy); fails on a factor < 1 or above
   the limit of 2^22 coarse cells. */
int heat_coarse_dims(int64_t nx, int64_t ny, int64_t fx, int64_t fy, int64_t* cr, int64_t* cc);
/* MERGE the lx x ly block whose cell (0,0) is cell (ox, oy) of an nx x ny plate
   into caller-owned CR*CC planes (initialised to 0, +inf, -inf; disjoint blocks
   add up): the device kernel on device planes, enqueued on `stream` without
   waiting, and its host twin on host memory. */
int heat_op_coarse(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                   int64_t oy, int64_t nx, int64_t ny, int64_t fx, int64_t fy, double* sum,
                   float* min, float* max, void* stream);
int heat_cpu_coarse(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                    int64_t oy, int64_t nx, int64_t ny, int64_t fx, int64_t fy, double* sum,
                    float* min, float* max);
/* The launch plan heat_op_coarse takes for a block (heat::gpu::coarse_plan) with
   the planner's constants, and a cap on the waves of a launch (0 = default) for
   tests that want every loop of the kernel to run more than once. */
typedef struct heat_coarse_plan {
  int64_t strips, chunks, units;
  int32_t owned, cells_per_strip, chunk_rows, cells_per_chunk, pieces, waves, vector_rows;
  int32_t strip_cols, max_chunk_rows, min_chunk_rows, waves_per_cu; /* constants */
  int32_t pad_;
} heat_coarse_plan;
int heat_op_coarse_plan(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                        int64_t oy, int64_t fx, int64_t fy, heat_coarse_plan* out);
int heat_op_coarse_max_waves(int waves);
/* Kernels alone, for timing (tools/coarse_bench.py): the merge into planes of
   keys (heat::gpu::CoarsePlanes: sum, key(-min), key(max)), their reset, and the
   checksum kernel accumulating into a caller-owned 32-byte device record.  No
   allocation, copy or wait. */
int heat_op_coarse_raw(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                       int64_t oy, int64_t nx, int64_t ny, int64_t fx, int64_t fy, double* sum,
                       int32_t* nmin_key, int32_t* max_key, void* stream);
int heat_op_coarse_reset(double* sum, int32_t* nmin_key, int32_t* max_key, int64_t cells,
                         void* stream);
int heat_op_checksum_raw(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                         int64_t oy, int64_t ny, void* record, void* stream);
/* Refinement (heat/io.hpp holds the definition).  The table of an axis of n cells
   refined by f: n entries each of i0, i1 (int32) and w (fp32). */
int heat_refine_axis(int64_t n, int64_t f, int order, int wrap, int32_t* i0, int32_t* i1,
                     float* w);
/* Fill the lx x ly block whose cell (0,0) is cell (ox, oy) of an nx x ny plate from
   the cr x cc grid S; `wrap`: the axes that wrap (1 x, 2 y), the others clamp.
   heat_op_refine: block and S in device memory; it builds and uploads the tables,
   enqueues the kernel on `stream` and waits for it before it frees them.
   heat_cpu_refine: the host twin on host memory. */
int heat_op_refine(float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox, int64_t oy,
                   int64_t nx, int64_t ny, const float* S, int64_t cr, int64_t cc, int64_t fx,
                   int64_t fy, int order, int wrap, void* stream);
int heat_cpu_refine(float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox, int64_t oy,
                    int64_t nx, int64_t ny, const float* S, int64_t cr, int64_t cc, int64_t fx,
                    int64_t fy, int order, int wrap);
/* The kernel alone, for timing (tools/refine_bench.py): S and the tables of the
   block's lx rows and ly columns already in device memory.  No allocation, copy
   or wait. */
int heat_op_refine_raw(float* origin, int64_t pitch, int64_t lx, int64_t ly, const float* S,
                       int64_t cc, const int32_t* ri0, const int32_t* ri1, const float* rw,
                       const int32_t* cj0, const int32_t* cj1, const float* cw, void* stream);
/* The launch plan heat_op_refine takes for a block (heat::gpu::refine_plan) with the
   planner's constants, and a cap on the waves of a launch (0 = default) for tests that
   want every loop of the kernel to run more than once. */
typedef struct heat_refine_plan {
  int64_t strips, chunks, units;
  int32_t chunk_rows, waves, align, vector_rows;
  int32_t strip_cols, max_chunk_rows, min_chunk_rows, waves_per_cu; /* constants */
} heat_refine_plan;
int heat_op_refine_plan(const float* origin, int64_t pitch, int64_t lx, int64_t ly,
                        heat_refine_plan* out);
int heat_op_refine_max_waves(int waves);
/* Mirror an lx x ly field into its `depth`-deep ghost frame beyond the insulated
   sides in `sides` (1 north, 2 south, 4 west, 8 east): the device kernel, and
   its host twin on host memory. */
int heat_op_fill_insulated_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int sides,
                                  int depth, void* stream);
int heat_cpu_fill_insulated_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly,
                                   int sides, int depth);
/* The general fill of the `depth`-deep ghost frame: the mirror image beyond the
   sides in `insulated_sides`, the field's opposite edge beyond both sides of the
   axes in `periodic_axes` (1 x, 2 y); an axis cannot have both.  Device kernel
   and host twin. */
int heat_op_fill_edge_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly,
                             int insulated_sides, int periodic_axes, int depth, void* stream);
int heat_cpu_fill_edge_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly,
                              int insulated_sides, int periodic_axes, int depth);
int heat_layout(int64_t lx, int64_t ly, int halo, int64_t* pitch, int64_t* rows, int* hx,
                int* hy);
int heat_tb_supported(int depth);
/* 1 once libheat_exp.so (the experiment kernels, `make exp`) has registered them. */
int heat_tb_exp_loaded(void);
/* The resident tile plan of a rows x cols box at `depth` as rows << 8 | waves
   (0: none): the device planner (device = 1, needs a GPU) or its host mirror
   (device = 0, what `heat --plan` uses). */
int heat_resident_shape(int64_t rows, int64_t cols, int depth, int device, int32_t* shape);

#ifdef __cplusplus
}
#endif

#endif /* HEAT_CAPI_H */
