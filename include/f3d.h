/*
 * f3d.h -- C ABI of libf3d_hip.so, the MI355X (gfx950) device library behind the
 * axruff/cuda-flow3d operator surface (src/cuda_operations/entire_data/ and src/optical_flow/optical_flow_e.{h,cpp}).
 *
 * The reference's operator hosts talk to the GPU through the CUDA *driver* API: cuModuleLoad of
 * kernels/<name>.ptx, cuModuleGetFunction, cuModuleGetGlobal("container_size"), cuLaunchKernel(args[]),
 * cuMemAllocPitch, cuMemcpy3D, cuMemsetD2D8, cuEvent*.  Every one of those uses on the hot path maps to
 * one entry point below; the comment on each cites the reference call site it replaces.
 *
 * Conventions
 *   - plain C types only: pointers, sizes, floats.  Device pointers are 64-bit integers (f3d_devptr),
 *     the same width as the CUdeviceptr values that travel through the reference's OperationParameters bag.
 *   - every function returns 0 on success, non-zero on failure; f3d_last_error() gives the message
 *     (thread local).  Nothing here throws and nothing silently falls back to a CPU path.
 *   - all device work is enqueued on one library-owned HIP stream, in order (the reference uses the NULL
 *     stream).  Launchers do not synchronise; call f3d_stream_sync().
 *   - volumes live in pitched "containers" addressed ((z - z_base) * container.height + y) * (pitch/4) + x
 *     (reference IND macro, src/kernels/solve_3d.cu:26); coarse pyramid levels occupy the corner sub-box.
 *     f3d_set_container() replaces the per-module __constant__ container_size upload.
 *   - `slab` (nullable) restricts a launcher to global planes [z_lo, z_hi) of a container whose plane 0
 *     holds global plane z_base; `depth` is always the GLOBAL depth of the level, so mirror / zero-padding
 *     rules are those of the whole volume.  NULL means the whole volume (z_base 0, planes [0, depth)).
 */
#ifndef F3D_H_
#define F3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint64_t f3d_devptr;

/* src/data_types/data_structs.h:20-25 (DataSize4; pitch in bytes) */
typedef struct f3d_size4 {
  size_t width;
  size_t height;
  size_t depth;
  size_t pitch;
} f3d_size4;

typedef struct f3d_slab {
  int z_base; /* global z held by container plane 0 */
  int z_lo;   /* first global plane to produce       */
  int z_hi;   /* one past the last plane to produce  */
} f3d_slab;

typedef struct f3d_event_s* f3d_event;
typedef struct f3d_queue_s* f3d_queue; /* a side stream for copies; NULL always means the library stream */

/* ---- runtime: context, memory, copies, events ------------------------------------------------ */

/* cuInit + cuDeviceGet + cuCtxCreate: src/utils/cuda_utils.cpp:21-57.  device < 0 picks LOCAL_RANK or 0. */
int f3d_init(int device);
/* cuCtxDestroy: src/main.cpp:236.  Idempotent: drains the library stream, destroys the timing events and the stream.
 * Memory is the owners' to free first (f3d_free, the operators' and drivers' Destroy). */
int f3d_shutdown(void);
/* 1 between a successful f3d_init() and f3d_shutdown(), else 0 (exit-time code asks before it touches the device) */
int f3d_is_initialized(void);
/* Lanes (no reference counterpart: the reference has one context and the NULL stream, src/utils/cuda_utils.cpp:21-57).  Every call
 * below that says "library stream", and f3d_set_container / f3d_set_conv_taps, act on the LANE of the calling thread: by default the
 * one lane the library creates in f3d_init.  A driver that is to run beside another one in the same process -- two frame pairs of a
 * sequence of small volumes solved at once (bin/flow3d --concurrent) -- creates a lane of its own (a stream, a container geometry, blur
 * taps) and makes it current in the thread that drives it; launches of different lanes are not ordered with each other.  Allocation,
 * events, queues and host registration are lane-agnostic; the profiling bracket (f3d_prof_*), the communicator and the out-of-core arena
 * belong to the default lane. */
typedef struct f3d_lane_s* f3d_lane;
int f3d_lane_create(f3d_lane* lane);
int f3d_lane_make_current(f3d_lane lane);   /* for the calling thread; NULL = back to the default lane */
int f3d_lane_is_private(void);              /* 1 when the calling thread is on a lane of its own */
int f3d_lane_get_current(f3d_lane* lane);   /* the calling thread's lane (NULL = the default one): code that borrows the thread for
                                               another lane puts this one back afterwards */
int f3d_lane_destroy(f3d_lane lane);        /* waits for the lane's stream first */

/* Diagnostics (no reference counterpart): from now on a fatal signal (SIGSEGV, SIGBUS, SIGILL, SIGFPE, SIGABRT) first writes
 * the signal number, the fault address and /proc/self/maps to `path`, then hands the signal to the handler that was installed
 * before (Python's faulthandler, a profiler's, the default action), so that the frames of a native stack trace can be resolved
 * to libraries.  Needs no device; calling it again only changes the file name. */
int f3d_crash_maps_enable(const char* path);
/* cuDeviceGetCount / cuDeviceGetName: src/utils/cuda_utils.cpp:27,44 */
int f3d_device_count(int* count);
int f3d_device_name(char* name, size_t capacity);
/* cuMemGetInfo: src/optical_flow/optical_flow_e.cpp:83 */
int f3d_mem_info(size_t* free_bytes, size_t* total_bytes);
/* cuDeviceGetAttribute(MAX_SHARED_MEMORY_PER_BLOCK): src/cuda_operations/entire_data/cuda_operation_solve.cpp:147 */
int f3d_lds_per_workgroup(int* bytes);
const char* f3d_last_error(void);

/* cuMemAllocPitch: src/optical_flow/optical_flow_e.cpp:104-108 (pitch is a multiple of 256 B) */
int f3d_alloc_pitched(f3d_devptr* ptr, size_t* pitch, size_t width_bytes, size_t rows);
/* cuMemFree: src/optical_flow/optical_flow_e.cpp:612 */
int f3d_free(f3d_devptr ptr);
/* cuMemsetD2D8: src/optical_flow/optical_flow_e.cpp:305-310, cuda_operation_solve.cpp:183-188 */
int f3d_memset2d(f3d_devptr ptr, size_t pitch, int value, size_t width_bytes, size_t rows);
/* cuMemcpy3D host->device / device->host, dense host volume <-> pitched container:
 * src/utils/cuda_utils.cpp:59-101.  depth planes are copied starting at container plane dev_plane0. */
int f3d_copy3d_h2d(f3d_devptr dst, size_t dev_pitch, size_t dev_height, size_t dev_plane0,
                   const float* src, size_t width, size_t height, size_t depth);
int f3d_copy3d_d2h(float* dst, size_t width, size_t height, size_t depth,
                   f3d_devptr src, size_t dev_pitch, size_t dev_height, size_t dev_plane0);
/* The piecemeal operators' chunk copies (cuMemcpy3D with srcZ / dstZ and host strides,
 * src/cuda_operations/partial_data/cuda_operation_solve_p.cpp:217-243, 278-296): `depth` planes of a width x height
 * region between a host volume whose rows are *_row_floats apart and whose planes are *_rows rows apart (the pointer
 * already addresses the first plane) and container planes dev_plane0...  Asynchronous on the library stream; order
 * reuse of the host memory with f3d_stream_sync(). */
int f3d_copy_planes_h2d(f3d_devptr dst, size_t dev_pitch, size_t dev_height, size_t dev_plane0, const float* src,
                        size_t src_row_floats, size_t src_rows, size_t width, size_t height, size_t depth);
int f3d_copy_planes_d2h(float* dst, size_t dst_row_floats, size_t dst_rows, size_t width, size_t height, size_t depth,
                        f3d_devptr src, size_t dev_pitch, size_t dev_height, size_t dev_plane0);
/* Copy queues: the piecemeal solver uploads the next chunk and downloads the previous one beside the kernels of the current
 * one.  Work on a queue is ordered; order BETWEEN queues (and the library stream, queue == NULL) is expressed with events:
 * f3d_event_record_on(ev, a); f3d_queue_wait_event(b, ev) makes everything issued to b afterwards wait for what a had been
 * given before the record.  (The reference has one NULL stream and synchronous cuMemcpy3D, cuda_operation_solve_p.cpp:226.) */
int f3d_queue_create(f3d_queue* queue);
int f3d_queue_destroy(f3d_queue queue);
int f3d_queue_sync(f3d_queue queue);
int f3d_event_record_on(f3d_event ev, f3d_queue queue);
int f3d_queue_wait_event(f3d_queue queue, f3d_event ev);
int f3d_copy_planes_h2d_on(f3d_queue queue, f3d_devptr dst, size_t dev_pitch, size_t dev_height, size_t dev_plane0, const float* src,
                           size_t src_row_floats, size_t src_rows, size_t width, size_t height, size_t depth);
int f3d_copy_planes_d2h_on(f3d_queue queue, float* dst, size_t dst_row_floats, size_t dst_rows, size_t width, size_t height,
                           size_t depth, f3d_devptr src, size_t dev_pitch, size_t dev_height, size_t dev_plane0);
/* width x height x depth floats between two containers of different geometry (pitch in bytes, rows per plane), on the
 * library stream: moves a chunk staged in one geometry into a resident container of another */
int f3d_copy_rect_d2d(f3d_devptr dst, size_t dst_pitch, size_t dst_rows, size_t dst_plane0, f3d_devptr src, size_t src_pitch,
                      size_t src_rows, size_t src_plane0, size_t width, size_t height, size_t depth);
/* Page-lock caller memory so the copies above run at full link rate and asynchronously (the reference's
 * ALLOCATE_PINNED_MEMORY switch, src/data_types/data3d.cpp:30,57-61, applied to memory the caller already owns). */
int f3d_host_register(void* ptr, size_t bytes);
int f3d_host_unregister(void* ptr);
/* *yes = 1 when ptr lies in page-locked host memory (registered here or allocated pinned by the caller) */
int f3d_host_is_pinned(const void* ptr, int* yes);
/* cuMemcpyDtoD: src/cuda_operations/entire_data/cuda_operation_median.cpp:96-98 */
int f3d_copy_d2d(f3d_devptr dst, f3d_devptr src, size_t bytes);
/* cuModuleGetGlobal("container_size") + cuMemcpyHtoD in every op's Initialize, e.g. cuda_operation_solve.cpp:59-61 */
int f3d_set_container(const f3d_size4* container);
/* the geometry last set (operators that switch it for a chunk put it back afterwards) */
int f3d_get_container(f3d_size4* container);

/* cuEventCreate/Record/Synchronize/ElapsedTime/Destroy: optical_flow_e.cpp:163-169,579-587 */
int f3d_event_create(f3d_event* ev);
int f3d_event_record(f3d_event ev);
int f3d_event_sync(f3d_event ev);
int f3d_event_elapsed_ms(float* ms, f3d_event start, f3d_event stop);
int f3d_event_destroy(f3d_event ev);
/* cuStreamSynchronize(NULL): cuda_operation_solve.cpp:257 */
int f3d_stream_sync(void);

/* ---- kernel launchers (one per reference __global__; same scalar lists as the reference arg arrays) -- */

/* compute_phi_ksi_3d, 18 args: cuda_operation_solve.cpp:195-213; kernel src/kernels/solve_3d.cu:33-262 */
int f3d_phi_ksi(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw,
                size_t width, size_t height, size_t depth, float hx, float hy, float hz,
                float equation_smoothness, float equation_data, f3d_devptr phi, f3d_devptr ksi,
                const f3d_slab* slab);

/* compute_phi_ksi_3d on TWO disjoint windows of the same container in one launch: the two zones of a z-slab whose weights had
 * to wait for the neighbours' increments (host/optical_flow_slab.cpp: CompleteWeights) -- two launches of a few planes each
 * otherwise.  Same results as two f3d_phi_ksi calls; an empty window falls back to one. */
int f3d_phi_ksi_zones(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                      f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, size_t width, size_t height, size_t depth, float hx,
                      float hy, float hz, float equation_smoothness, float equation_data, f3d_devptr phi, f3d_devptr ksi,
                      const f3d_slab* zone_a, const f3d_slab* zone_b);

/* solve_3d, 20 args: cuda_operation_solve.cpp:224-244; kernel src/kernels/solve_3d.cu:264-508.
 * One Jacobi sweep (in-voxel Gauss-Seidel du->dv->dw) into temp_d*; the caller ping-pongs the buffers. */
int f3d_solve_sweep(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                    f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi, f3d_devptr ksi,
                    size_t width, size_t height, size_t depth, float hx, float hy, float hz, float equation_alpha,
                    f3d_devptr temp_du, f3d_devptr temp_dv, f3d_devptr temp_dw, const f3d_slab* slab);

/* The LAST sweep of a level with the flow update in it: f3d_solve_sweep whose three outputs receive flow_u + du', flow_v + dv',
 * flow_w + dw' (du', dv', dw' being what f3d_solve_sweep would have written; one binary32 add each) -- bit for bit what
 * f3d_solve_sweep followed by f3d_add(flow_*, temp_d*) leaves in flow_*, without the nine array passes of the add: the sweep has
 * both operands in registers.  Same arguments, slab window and refusals as f3d_solve_sweep; in addition an output that is also one of
 * the ten inputs is refused.  flow_* and flow_d* are not written. */
int f3d_solve_sweep_add(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                        f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi, f3d_devptr ksi,
                        size_t width, size_t height, size_t depth, float hx, float hy, float hz, float equation_alpha,
                        f3d_devptr sum_u, f3d_devptr sum_v, f3d_devptr sum_w, const f3d_slab* slab);

/* TWO consecutive solve_3d sweeps in one launch: temp_d* receive what two f3d_solve_sweep calls with a buffer swap in
 * between would leave in flow_d* (bit for bit); the intermediate field never goes to HBM, so the pair moves the bytes of
 * one sweep.  Replaces two iterations of the inner loop of cuda_operation_solve.cpp:222-255; the caller swaps ONCE.
 * A slab window [z_lo, z_hi) needs planes z_lo-2 .. z_hi+1 of every input inside the container.
 * RESTRICTION of every fused entry (f3d_solve_sweep2, f3d_solve_sweep_phi_ksi[_edges] and their _fd forms): the three face weights
 * equation_alpha / (h * h) must be finite and not negative -- the kernels select w or +0 where solve_3d.cu:437-445 multiplies by
 * (float)(flag), which is the same float only then; other parameters are refused (status 1, f3d_last_error says so) and the
 * caller uses f3d_solve_sweep / f3d_phi_ksi, which multiply like the reference (the host operators do that by themselves). */
int f3d_solve_sweep2(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                     f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi, f3d_devptr ksi,
                     size_t width, size_t height, size_t depth, float hx, float hy, float hz, float equation_alpha,
                     f3d_devptr temp_du, f3d_devptr temp_dv, f3d_devptr temp_dw, const f3d_slab* slab);

/* The last solve_3d sweep of an outer iteration AND compute_phi_ksi_3d of the next one in one launch: temp_d* receive the
 * sweep (what f3d_solve_sweep would write), phi_next / ksi_next what f3d_phi_ksi would then compute from temp_d* -- bit for
 * bit; the kernel reads frame_0 .. ksi once for both.  Replaces the launch pair cuda_operation_solve.cpp:246-252 (last j) +
 * :215-221 (next i).  phi_next / ksi_next must be buffers of their own: other tiles are still reading phi / ksi while this
 * launch writes (the operator ping-pongs two pairs).  A slab window [z_lo, z_hi) needs planes z_lo-2 .. z_hi+1 of every input
 * inside the container; the container pitch must be a multiple of 256 bytes. */
int f3d_solve_sweep_phi_ksi(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                            f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi, f3d_devptr ksi,
                            size_t width, size_t height, size_t depth, float hx, float hy, float hz, float equation_alpha,
                            float equation_smoothness, float equation_data, f3d_devptr temp_du, f3d_devptr temp_dv,
                            f3d_devptr temp_dw, f3d_devptr phi_next, f3d_devptr ksi_next, const f3d_slab* slab);

/* The same launch for a z-slab that exchanges its increments AFTER it (host/optical_flow_slab.cpp): the sweep is computed on
 * planes z_lo-1 .. z_hi anyway (the weights of z_lo and z_hi-1 need it); keep_below / keep_above also STORE it there, so a rank
 * launches on the window [own.lo + 1, own.hi - 1) and ends up with the sweep on all of its planes and the next weights on all
 * but the two whose neighbours it does not have yet (those follow from f3d_phi_ksi once the halo planes have arrived).  Planes
 * outside the volume do not exist: keep_below at z_lo = 0 and keep_above at z_hi = depth are ignored. */
int f3d_solve_sweep_phi_ksi_edges(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                                  f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi, f3d_devptr ksi,
                                  size_t width, size_t height, size_t depth, float hx, float hy, float hz, float equation_alpha,
                                  float equation_smoothness, float equation_data, f3d_devptr temp_du, f3d_devptr temp_dv,
                                  f3d_devptr temp_dw, f3d_devptr phi_next, f3d_devptr ksi_next, const f3d_slab* slab,
                                  int keep_below, int keep_above);

/* 1 when f3d_solve_sweep2 / f3d_solve_sweep_phi_ksi on a level of this size (whole volume, current container) take the tile that marches
 * along y with every z plane in it -- thin volumes, BASELINE config 3 -- which exists for the entry points on FRAMES only: a caller that
 * would otherwise read frame derivatives (the _fd entries march along z) is better off on the frames there.  Pure geometry, no launch. */
int f3d_fused_launches_march_along_y(size_t width, size_t height, size_t depth);

/* THREE consecutive solve_3d sweeps in one launch (k_tri, csrc/f3d_solve_tri.h): temp_d* receive what three f3d_solve_sweep calls with
 * the buffer swaps in between would leave, bit for bit.  Replaces three iterations of the inner loop of
 * cuda_operation_solve.cpp:222-255; the caller swaps ONCE.  For small and mid-size levels, where a launch is bound by its own
 * skeleton and a third stage costs a fifth of it (profiles/r04_three_stage_probe.txt); the fused-entry restriction on alpha / h^2
 * holds.  A slab window [z_lo, z_hi) needs planes z_lo-3 .. z_hi+2 of every input inside the container; the container pitch must be a
 * multiple of 256 bytes; no output may be one of the inputs. */
int f3d_solve_sweep3(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                     f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi, f3d_devptr ksi, size_t width,
                     size_t height, size_t depth, float hx, float hy, float hz, float equation_alpha, f3d_devptr temp_du,
                     f3d_devptr temp_dv, f3d_devptr temp_dw, const f3d_slab* slab);
/* The last TWO sweeps of an outer iteration and compute_phi_ksi_3d of the next one in one launch: temp_d* receive the second sweep,
 * phi_next / ksi_next what f3d_phi_ksi would then compute from temp_d* (cuda_operation_solve.cpp:246-252 twice + :215-221 of the next
 * i).  With the default five sweeps an outer iteration is f3d_solve_sweep3 + f3d_solve_sweep2_phi_ksi: two launches for the
 * reference's six.  Same conditions as f3d_solve_sweep3; phi_next / ksi_next must be buffers of their own. */
int f3d_solve_sweep2_phi_ksi(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                             f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi, f3d_devptr ksi, size_t width,
                             size_t height, size_t depth, float hx, float hy, float hz, float equation_alpha,
                             float equation_smoothness, float equation_data, f3d_devptr temp_du, f3d_devptr temp_dv,
                             f3d_devptr temp_dw, f3d_devptr phi_next, f3d_devptr ksi_next, const f3d_slab* slab);

/* The frame derivatives of a level, once: fx, fy, fz = (((F0[+1] - F0[-1]) + F1[+1]) - F1[-1]) / (4 h) and ft = F1 - F0, exactly as
 * compute_phi_ksi_3d and solve_3d form them for every voxel in every launch (src/kernels/solve_3d.cu:205-215, :438-448).  They depend
 * on the two frames of the level only; the _fd launchers below read them instead of the frames.  A slab window [z_lo, z_hi) needs planes
 * z_lo-1 .. z_hi of both frames inside the container. */
int f3d_frame_derivatives(f3d_devptr frame_0, f3d_devptr frame_1, size_t width, size_t height, size_t depth, float hx, float hy,
                          float hz, f3d_devptr fx, f3d_devptr fy, f3d_devptr fz, f3d_devptr ft, const f3d_slab* slab);
/* f3d_solve_sweep2 and f3d_solve_sweep_phi_ksi on precomputed frame derivatives (same results bit for bit; the four derivative
 * volumes must cover the planes the frames would have had to: z_lo-1 .. z_hi for a window [z_lo, z_hi)). */
int f3d_solve_sweep2_fd(f3d_devptr fx, f3d_devptr fy, f3d_devptr fz, f3d_devptr ft, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
                        f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi, f3d_devptr ksi, size_t width,
                        size_t height, size_t depth, float hx, float hy, float hz, float equation_alpha, f3d_devptr temp_du,
                        f3d_devptr temp_dv, f3d_devptr temp_dw, const f3d_slab* slab);
int f3d_solve_sweep_phi_ksi_fd(f3d_devptr fx, f3d_devptr fy, f3d_devptr fz, f3d_devptr ft, f3d_devptr flow_u, f3d_devptr flow_v,
                               f3d_devptr flow_w, f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi,
                               f3d_devptr ksi, size_t width, size_t height, size_t depth, float hx, float hy, float hz,
                               float equation_alpha, float equation_smoothness, float equation_data, f3d_devptr temp_du,
                               f3d_devptr temp_dv, f3d_devptr temp_dw, f3d_devptr phi_next, f3d_devptr ksi_next, const f3d_slab* slab);
/* ... and f3d_solve_sweep_phi_ksi_edges on frame derivatives (the z-slab driver: derivative volumes per slab, computed once per level on
 * the slab widened by the halo depth minus one) */
int f3d_solve_sweep_phi_ksi_edges_fd(f3d_devptr fx, f3d_devptr fy, f3d_devptr fz, f3d_devptr ft, f3d_devptr flow_u, f3d_devptr flow_v,
                                     f3d_devptr flow_w, f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi,
                                     f3d_devptr ksi, size_t width, size_t height, size_t depth, float hx, float hy, float hz,
                                     float equation_alpha, float equation_smoothness, float equation_data, f3d_devptr temp_du,
                                     f3d_devptr temp_dv, f3d_devptr temp_dw, f3d_devptr phi_next, f3d_devptr ksi_next,
                                     const f3d_slab* slab, int keep_below, int keep_above);

/* WEIGHTS FIRST: compute_phi_ksi_3d of an outer iteration AND its first solve_3d sweep in one launch (k_wpair8): phi_out / ksi_out
 * receive what f3d_phi_ksi computes from flow_* and flow_d*, temp_d* what f3d_solve_sweep then computes with those weights -- bit for
 * bit.  The weights are outputs only: the launch reads ten volumes and writes five.  Whole levels only.  The entry DECLINES -- status 1,
 * f3d_last_error says why, nothing is launched or written -- on a slab window, on a level the fused launches march along y
 * (f3d_fused_launches_march_along_y), on a container pitch that is not a multiple of 256 floats, on face weights that are not plain
 * (the fused-entry restriction above) and when an output is also an input; the caller then takes f3d_phi_ksi and the sweeps. */
int f3d_solve_phi_ksi_sweep_fd(f3d_devptr fx, f3d_devptr fy, f3d_devptr fz, f3d_devptr ft, f3d_devptr flow_u, f3d_devptr flow_v,
                               f3d_devptr flow_w, f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, size_t width, size_t height,
                               size_t depth, float hx, float hy, float hz, float equation_alpha, float equation_smoothness,
                               float equation_data, f3d_devptr phi_out, f3d_devptr ksi_out, f3d_devptr temp_du, f3d_devptr temp_dv,
                               f3d_devptr temp_dw, const f3d_slab* slab);
/* f3d_solve_sweep2_fd whose outputs receive flow_u + du'', flow_v + dv'', flow_w + dw'' (one binary32 add each): the last launch of a
 * level with the flow update in it, the two-sweep counterpart of f3d_solve_sweep_add.  Declines as the entry above does. */
int f3d_solve_sweep2_add_fd(f3d_devptr fx, f3d_devptr fy, f3d_devptr fz, f3d_devptr ft, f3d_devptr flow_u, f3d_devptr flow_v,
                            f3d_devptr flow_w, f3d_devptr flow_du, f3d_devptr flow_dv, f3d_devptr flow_dw, f3d_devptr phi, f3d_devptr ksi,
                            size_t width, size_t height, size_t depth, float hx, float hy, float hz, float equation_alpha, f3d_devptr sum_u,
                            f3d_devptr sum_v, f3d_devptr sum_w, const f3d_slab* slab);

/* registration_3d, 12 args: cuda_operation_registration.cpp:110-122; kernel src/kernels/registration_3d.cu:28-82.
 * output must not be frame_1 (every voxel gathers from other voxels of it; refused, as cuda_operation_registration.cpp:100-103 does).
 * output may be frame_0: a voxel reads only its own voxel of frame_0, before it writes, and the reference's operator allows it. */
int f3d_warp(f3d_devptr frame_0, f3d_devptr frame_1, f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w,
             size_t width, size_t height, size_t depth, float hx, float hy, float hz, f3d_devptr output,
             const f3d_slab* slab);

/* resample_{x,y,z}_3d, 6 args: cuda_operation_resample.cpp:115-120,138-143,161-166; src/kernels/resample_3d.cu.
 * slab_in describes the input container (z pass only reads through it), slab the output planes.
 * The x pass takes one of three kernels with the same bits: rows of up to 1024 floats resampled to up to 1024 outputs are walked
 * several per wave with the output windows held in registers (k_resample_x_rows), longer rows of up to 2048 floats are staged one
 * per wave (k_resample_x_lds), and anything else -- longer rows, rows that do not start 16-byte aligned -- reads global memory
 * directly (k_resample<0>). */
int f3d_resample_x(f3d_devptr input, f3d_devptr output, size_t out_width, size_t out_height, size_t out_depth,
                   size_t in_width, const f3d_slab* slab);
int f3d_resample_y(f3d_devptr input, f3d_devptr output, size_t out_width, size_t out_height, size_t out_depth,
                   size_t in_height, const f3d_slab* slab);
int f3d_resample_z(f3d_devptr input, f3d_devptr output, size_t out_width, size_t out_height, size_t out_depth,
                   size_t in_depth, const f3d_slab* slab_in, const f3d_slab* slab);

/* add_3d, 5 args: cuda_operation_add.cpp:86-91; src/kernels/add_3d.cu:26-41 */
int f3d_add(f3d_devptr operand_0, f3d_devptr operand_1, size_t width, size_t height, size_t depth,
            const f3d_slab* slab);

/* median_3d, 6 args: cuda_operation_median.cpp:131-137; src/kernels/median_3d.cu:49-299.
 * radius is the window DIAMETER, one of 3, 5, 7 (the host op applies the 1 / even rules). */
int f3d_median(f3d_devptr input, size_t width, size_t height, size_t depth, size_t radius, f3d_devptr output,
               const f3d_slab* slab);

/* Up to three volumes of ONE box in one launch (extensions, no cu* site of their own): the reference runs "+=", the median and the
 * three resampling passes once per flow component and frame (optical_flow_e.cpp:274-345, 420-473); the components do not depend
 * on each other there, and on levels below ~128^3 a launch is mostly fixed cost.  Element i of every array belongs to volume i;
 * the kernels, arguments and results are those of the single-volume entries above (which are the count = 1 case of these).  No
 * input of a batch may be an output of the same batch.  count = 1 .. 3. */
int f3d_resample_x_n(const f3d_devptr* inputs, const f3d_devptr* outputs, size_t count, size_t out_width, size_t out_height,
                     size_t out_depth, size_t in_width, const f3d_slab* slab);
int f3d_resample_y_n(const f3d_devptr* inputs, const f3d_devptr* outputs, size_t count, size_t out_width, size_t out_height,
                     size_t out_depth, size_t in_height, const f3d_slab* slab);
int f3d_resample_z_n(const f3d_devptr* inputs, const f3d_devptr* outputs, size_t count, size_t out_width, size_t out_height,
                     size_t out_depth, size_t in_depth, const f3d_slab* slab_in, const f3d_slab* slab);
int f3d_add_n(const f3d_devptr* operand_0, const f3d_devptr* operand_1, size_t count, size_t width, size_t height, size_t depth,
              const f3d_slab* slab);
int f3d_median_n(const f3d_devptr* inputs, size_t count, size_t width, size_t height, size_t depth, size_t radius,
                 const f3d_devptr* outputs, const f3d_slab* slab);
/* The box width x height x [slab planes] of up to three volumes of the current container set to +0.f in one launch: the
 * increments du, dv, dw at the start of a level's solve.  The reference clears every row of every plane of the container there
 * (three cuMemsetD2D8, cuda_operation_solve.cpp:183-188); nothing ever reads a row or plane outside the level's box -- every
 * kernel mirrors by address inside it -- so only the box is written. */
int f3d_clear_box_n(const f3d_devptr* volumes, size_t count, size_t width, size_t height, size_t depth, const f3d_slab* slab);

/* c_Kernel upload: cuda_operation_convolution.cpp:160-161 (at most 51 taps, MAX_KERNEL_LENGTH) */
int f3d_set_conv_taps(const float* taps, size_t count);
/* convolution{Rows,Columns,Slices}Kernel, 7 args: cuda_operation_convolution.cpp:221-228,274-281,327-334;
 * src/kernels/convolution_3d.cu:75-172,186-271,284-372.  Zero padding; taps from f3d_set_conv_taps. */
int f3d_conv_rows(f3d_devptr dst, f3d_devptr src, size_t width, size_t height, size_t depth, size_t kernel_radius,
                  const f3d_slab* slab);
int f3d_conv_cols(f3d_devptr dst, f3d_devptr src, size_t width, size_t height, size_t depth, size_t kernel_radius,
                  const f3d_slab* slab);
int f3d_conv_slices(f3d_devptr dst, f3d_devptr src, size_t width, size_t height, size_t depth, size_t kernel_radius,
                    const f3d_slab* slab);
/* convolutionRowsKernel followed by convolutionColumnsKernel in ONE launch (the two launches of
 * cuda_operation_convolution.cpp:172-177): dst receives what f3d_conv_rows into a scratch volume and f3d_conv_cols from it
 * would leave, bit for bit; the row-convolved volume only ever exists in LDS. */
int f3d_conv_rows_cols(f3d_devptr dst, f3d_devptr src, size_t width, size_t height, size_t depth, size_t kernel_radius,
                       const f3d_slab* slab);

/* Self-test (no reference counterpart): the fused sweep + phi/ksi kernel forms the weights 1 / (2 sqrt(a)) of
 * src/kernels/solve_3d.cu:203-204,259-260 by a shorter instruction sequence that has been checked against the IEEE square root and
 * division for EVERY argument it is used on.  This entry point repeats that check on the device it runs on: all bit patterns in
 * [lo_bits, hi_bits] (as floats), `excluded` = arguments the kernel sends down the IEEE road instead (outside 2^-100 .. 2^100, or
 * a root with an all-ones significand), `checked` = the rest, `mismatches` = how many of those differ from the IEEE chain (0 on
 * gfx950), first_mismatch = one such bit pattern.  tests/test_gpu_kernels.py sweeps the whole binary32 range. */
int f3d_selftest_weights(unsigned lo_bits, unsigned hi_bits, unsigned long long* checked, unsigned long long* excluded,
                         unsigned long long* mismatches, unsigned* first_mismatch);

/* ---- profiler ranges (no reference counterpart; SURVEY.md section 5 "tracing") ---------------------------------
 * roctx ranges around operators and pyramid levels so that rocprofv3 --marker-trace attributes kernels to them.
 * librocprofiler-sdk-roctx is dlopen'ed on the first push and only when F3D_ROCTX=1 is set or a rocprofiler tool library
 * is preloaded; otherwise both calls return at once.  Ranges nest; pop closes the innermost. */
int f3d_range_push(const char* name);
int f3d_range_pop(void);

/* ---- per-kernel timing (HIP events on the library stream), used by bench.py's roofline leg ----------- */

enum { F3D_K_PHI_KSI = 0, F3D_K_SWEEP = 1, F3D_K_SWEEP2 = 2, F3D_K_SWEEP_PHI_KSI = 3, F3D_K_SWEEP3 = 4, F3D_K_SWEEP2_PHI_KSI = 5,
       F3D_K_COUNT = 6 };
/* (id 3 is "a sweep and a phi/ksi in one launch", 92 algorithmic bytes per voxel, in either order: f3d_solve_sweep_phi_ksi* and
 * f3d_solve_phi_ksi_sweep_fd; id 2 is two sweeps, f3d_solve_sweep2* and f3d_solve_sweep2_add_fd) */
/* enable = 1 brackets every launch of the solver kernels (phi/ksi, one sweep, two fused sweeps) with events on the library stream */
int f3d_prof_enable(int enable);
int f3d_prof_reset(void);
/* which kernels get events while profiling is enabled: bit k = kernel id k (default all).  Two event records per launch
 * cost ~7 us of dispatch, 2 % of a 512^3 solve when all 6400 solver launches carry them */
int f3d_prof_select(unsigned kernel_mask);
/* drains the pending events; min_voxels filters launches by level size (0 = all) */
int f3d_prof_read(int kernel, size_t min_voxels, double* total_ms, uint64_t* launches, double* total_voxels);

/* ---- multi-GPU: z-slab halo exchange on RCCL over xGMI (no reference counterpart) --------- */

/* 128-byte ncclUniqueId, created on rank 0 and handed to the other ranks by the launcher (bench.py sends it
 * through torch.distributed).  librccl is loaded on the first of these calls, never for single-GPU use. */
int f3d_comm_unique_id(void* id128);
int f3d_comm_init(const void* id128, int rank, int n_ranks);
int f3d_comm_destroy(void);
int f3d_comm_rank(int* rank, int* n_ranks);
/* What the transport itself says (any pointer may be null): backend 0 = none, 1 = RCCL, 2 = the shared-memory rehearsal
 * transport; with RCCL comm_ranks / comm_rank / comm_device are the answers of ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice for the live communicator (-1 where the library lacks the query); sent_bytes / exchanges count what
 * this rank has handed to the transport since f3d_comm_init (bench.py reports them per run). */
int f3d_comm_info(int* backend, int* comm_ranks, int* comm_rank, int* comm_device, unsigned long long* sent_bytes,
                  unsigned long long* exchanges);
/* Gather `count` container planes (sub-box width x height of each) of `field`, starting at container plane
 * plane0, into the dense staging buffer at staging[offset_floats ...]; unpack is the inverse. */
int f3d_pack_planes(f3d_devptr field, int plane0, int count, size_t width, size_t height, f3d_devptr staging,
                    size_t offset_floats);
int f3d_unpack_planes(f3d_devptr field, int plane0, int count, size_t width, size_t height, f3d_devptr staging,
                      size_t offset_floats);
/* the same for up to 32 (field, plane range) segments in ONE launch: segment i covers count[i] planes of fields[i]
 * from container plane plane0[i] and sits at staging[offset_floats[i] ...] */
int f3d_pack_segments(const f3d_devptr* fields, const int* plane0, const int* count, const size_t* offset_floats,
                      int n_segments, size_t width, size_t height, f3d_devptr staging);
int f3d_unpack_segments(const f3d_devptr* fields, const int* plane0, const int* count, const size_t* offset_floats,
                        int n_segments, size_t width, size_t height, f3d_devptr staging);
/* same-device plane copy between two containers (one-GPU rehearsal of the slab decomposition) */
int f3d_copy_planes(f3d_devptr dst, int dst_plane0, f3d_devptr src, int src_plane0, int count, size_t width,
                    size_t height);
/* ... and up to any number of (destination, source, plane range) triples in as few launches as possible (32 per launch): a whole
 * in-process exchange -- every rank, peer and field -- instead of a launch per triple */
int f3d_copy_plane_segments(const f3d_devptr* dst, const int* dst_plane0, const f3d_devptr* src, const int* src_plane0, const int* count,
                            int n_segments, size_t width, size_t height);
/* One grouped exchange on the library stream: for every i, send send_count[i] floats from send_buf + send_offset[i]
 * to peers[i] and receive recv_count[i] floats into recv_buf + recv_offset[i] from peers[i] (zero counts skipped). */
int f3d_comm_sendrecv(f3d_devptr send_buf, const size_t* send_offset, const size_t* send_count, f3d_devptr recv_buf,
                      const size_t* recv_offset, const size_t* recv_count, const int* peers, int n_peers);
/* The same exchange split in two: _begin starts it behind everything issued on the library stream so far (on a side
 * stream, so kernels issued afterwards run beside it); _end makes the library stream wait for the received data.  The
 * send buffer must not be rewritten, nor the receive buffer read, in between.  One exchange may be open at a time. */
int f3d_comm_sendrecv_begin(f3d_devptr send_buf, const size_t* send_offset, const size_t* send_count, f3d_devptr recv_buf,
                            const size_t* recv_offset, const size_t* recv_count, const int* peers, int n_peers);
int f3d_comm_sendrecv_end(void);
/* Measured cost of an exchange (nothing in the reference to match: src/utils/cuda_utils.cpp:38,52 use one device).  While
 * f3d_comm_timing(1) is in force HIP events bracket three kinds of interval on the stream the work runs on:
 *   class 0  a whole blocking exchange -- the caller marks it: f3d_comm_mark(0, 0) before the pack launch, f3d_comm_mark(1, 0) after
 *            the unpack launch (host/optical_flow_slab.cpp: Exchange)
 *   class 1  the same marks around an exchange whose transfer runs beside kernels (f3d_comm_sendrecv_begin / _end with the
 *            interior in between): the interval includes the kernels it hides behind
 *   class 2  the grouped ncclSend / ncclRecv alone (recorded by the library on the stream it was posted to)
 * f3d_comm_timing(1) also clears the sums; f3d_comm_timing_read drains the streams and returns total / count / min / max in
 * microseconds and the bytes this rank sent inside the intervals.  Off by default; with it off f3d_comm_mark does nothing. */
int f3d_comm_timing(int enable);
int f3d_comm_mark(int what, int cls);
int f3d_comm_timing_read(int cls, double* total_us, unsigned long long* count, double* min_us, double* max_us,
                         unsigned long long* bytes);
/* max over all ranks of *value (host in/out) */
int f3d_comm_allreduce_max_f32(float* value);
/* max |field| over the slab's planes, on the device (feeds the warp halo depth) */
int f3d_abs_max(f3d_devptr field, size_t width, size_t height, size_t depth, const f3d_slab* slab, float* result);

/* Flow statistics on the device: min, max and SUM of sqrt(u^2 + v^2 + w^2) over the slab's planes (host out; the
 * caller divides by the voxel count, or adds the sums of several slabs first).  Device counterpart of the host loop
 * in src/cuda_operations/partial_data/cuda_operation_stat_p.cpp:85-104; min and max are exact, the sum is accumulated in
 * double (the reference adds floats in scan order). */
int f3d_flow_stats(f3d_devptr flow_u, f3d_devptr flow_v, f3d_devptr flow_w, size_t width, size_t height, size_t depth,
                   const f3d_slab* slab, float* min_magnitude, float* max_magnitude, double* sum_magnitude);

/* Registration residual on the device: sum of (warped - frame_0)^2, sum of |warped - frame_0| (both accumulated in double)
 * and max |warped - frame_0| over the slab's planes (host out).  The reference's counterpart is the disabled debug block of
 * src/optical_flow/optical_flow_e.cpp:536-571, which registers frame_1 with the final flow (cuop_register_, h = 1) and dumps
 * the volume for inspection; here the comparison with frame_0 is a reduction and nothing is written to disk. */
int f3d_residual_stats(f3d_devptr frame_0, f3d_devptr frame_1_warped, size_t width, size_t height, size_t depth,
                       const f3d_slab* slab, double* sum_squares, double* sum_abs, float* max_abs);

/* Trajectory step (no reference counterpart: the reference writes the flow of each consecutive pair, src/main.cpp:132-185).
 * acc = (acc_u, acc_v, acc_w) is the displacement of every voxel of frame 0 so far (frame 0's grid, voxel units); inc is the flow
 * of the next pair, defined on the grid of the frame the points have reached.  For every voxel (x, y, z), in place:
 *   p = (x + acc_u, y + acc_v, z + acc_w)            (one float add per axis)
 *   p NaN, or outside [0, width-1] x [0, height-1] x [0, depth-1]:  acc = (NaN, NaN, NaN)   (the point is lost and stays lost)
 *   else:  acc += inc sampled trilinearly at p       (f3d_warp's sample, src/kernels/registration_3d.cu:66-79, same order)
 * Starting from acc = 0 the first step gives inc back exactly.  Geometry from the current container (f3d_set_container), whole
 * volume, library stream.  No acc component may be an inc component.  lost (nullable): the number of voxels whose acc_u is NaN
 * after the step; asking for it waits for the stream, passing NULL does not. */
int f3d_compose_flow(f3d_devptr acc_u, f3d_devptr acc_v, f3d_devptr acc_w, f3d_devptr inc_u, f3d_devptr inc_v,
                     f3d_devptr inc_w, size_t width, size_t height, size_t depth, unsigned long long* lost);

/* A displacement made fit to start a solve from (no reference counterpart: the reference starts every pyramid from a flow of zero,
 * src/optical_flow/optical_flow_e.cpp:303-345).  (u, v, w) is a guess of the flow of a pair on frame 0's grid, voxel units: a coarse
 * DVC, an FE prediction, a rigid pre-registration, the flow of the pair before.  For every voxel (x, y, z) of the box:
 *   u, v and w all finite:  out = (u, v, w), the same bits (a -0 stays -0)
 *   else:                   out = (+0, +0, +0), and the voxel counts in `replaced`
 * info (nullable):
 *   voxels    width * height * depth
 *   replaced  as above
 *   leaving   the finite voxels whose end point (x + u, y + v, z + w) (one float add per axis, as in f3d_compose_flow) lies outside
 *             [0, width-1] x [0, height-1] x [0, depth-1]
 *   max_abs   the largest |component| over the finite voxels, 0 when there is none
 * All four are exact whatever the schedule (integer counts, a maximum).  out_u, out_v, out_w may be u, v, w themselves (component
 * for component); any other sharing between the six containers is refused.  Padding outside the box is neither read nor written.
 * Geometry from the current container (f3d_set_container), whole volume, library stream.  Asking for info waits for the stream,
 * passing NULL only enqueues.  Refused: a null container, a zero dimension, a box larger than the container. */
typedef struct f3d_initial_info {
  unsigned long long voxels, replaced, leaving;
  float max_abs;
} f3d_initial_info;
int f3d_initial_flow(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w, size_t width,
                     size_t height, size_t depth, f3d_initial_info* info);

/* Strain fields of a displacement (no reference counterpart: the deformation analysis a motion study does with the flows of
 * src/main.cpp:132-185).  d = (u, v, w) is a pair's flow or a cumulative displacement, voxel units.  G[r][c] = d d_r / d x_c
 * (row r = component 0 u, 1 v, 2 w; column c = axis 0 x, 1 y, 2 z), F = I + G.
 * Missing samples: a grid point is missing when it lies outside the volume or any of its three components is NaN.  For voxel p:
 *   p missing                          -> every output of p is NaN
 *   per axis a of size n:  n == 1      -> column a of G is 0
 *     else, m = p - e_a, q = p + e_a:  both present  G[:,a] = (d(q) - d(m)) * 0.5f
 *                                      only q        G[:,a] = d(q) - d(p)
 *                                      only m        G[:,a] = d(p) - d(m)
 *                                      neither       every output of p is NaN
 * Outputs, in this order (out[0..7]), selected by group:
 *   F3D_STRAIN_VOL  out[0] vol = J - 1 (J = det F)
 *   F3D_STRAIN_E    out[1..6] exx eyy ezz exy exz eyz: Green-Lagrange E = 1/2 (F^T F - I) (tensor components, not 2 exy)
 *   F3D_STRAIN_EQ   out[7] eq: equivalent (von Mises) strain of E
 * Every operation float32, rounded on its own, in exactly this order (G itself, not F, so small strains do not cancel against 1):
 *   I1  = (G00 + G11) + G22
 *   I2  = ((G00*G11 - G01*G10) + (G11*G22 - G12*G21)) + (G00*G22 - G02*G20)
 *   I3  = (G00*(G11*G22 - G12*G21) - G01*(G10*G22 - G12*G20)) + G02*(G10*G21 - G11*G20)
 *   vol = (I1 + I2) + I3
 *   E_rc = 0.5f * ((G_rc + G_cr) + ((G_0r*G_0c + G_1r*G_1c) + G_2r*G_2c))        (r, c in {0,1,2} = x,y,z)
 *   m = ((Exx + Eyy) + Ezz) / 3.f ;  a = Exx - m ;  b = Eyy - m ;  c = Ezz - m
 *   s = ((a*a + b*b) + c*c) + 2.f * ((Exy*Exy + Exz*Exz) + Eyz*Eyz)
 *   eq = sqrtf(s / 1.5f)
 * Geometry from the current container (f3d_set_container), whole volume, library stream.  Entries of out for groups not selected
 * are ignored and never written.  Refused: a null input; a null selected output; fields 0 or with unknown bits; a selected output
 * that is also an input; two selected outputs that are the same container.
 * stats (nullable; asking waits for the stream): defined = voxels whose vol is not NaN, folded = voxels with vol <= -1 (J <= 0),
 * vol_min / vol_max / eq_max over the defined voxels (exact; NaN when none is defined), vol_sum accumulated in double (0 when none).
 * vol and eq are computed for the statistics whether or not they are stored. */
#define F3D_STRAIN_VOL 1u
#define F3D_STRAIN_E 2u
#define F3D_STRAIN_EQ 4u
typedef struct f3d_strain_stats {
  unsigned long long defined, folded;
  float vol_min, vol_max, eq_max;
  double vol_sum;
} f3d_strain_stats;
int f3d_flow_strain(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[8], unsigned fields, size_t width,
                    size_t height, size_t depth, f3d_strain_stats* stats /* nullable; non-null waits */);

/* Strain fields of a displacement over a strain window: the displacement gradient G of a voxel is the slope of the unweighted
 * least-squares plane through the displacement samples of its (2 radius + 1)^3 neighbourhood, and the strain fields are formed from
 * that G by f3d_flow_strain's expressions.  It is a local affine fit of d itself, not a blur of strain fields: an affine displacement
 * is reproduced whatever the pattern of missing samples, at radius 1 on a full window G[r][a] is the mean of the nine central
 * differences around the voxel, and white noise of deviation s in d gives s / sqrt((2r+1)^2 sum i^2) in G (0.236 s, 0.063 s,
 * 0.027 s at radius 1, 2, 3, against 0.707 s of f3d_flow_strain).  The arithmetic below is part of the ABI.
 * Presence: a grid point is present when it lies inside the volume and none of u, v, w is NaN there (f3d_flow_strain's rule).  For
 * voxel p, over the offsets (i, j, k) in [-r, r]^3 from p, with m = 1 at a present point and 0 elsewhere:
 *   mask moments, exact integers:  n = sum m, Sx = sum i m, Sy = sum j m, Sz = sum k m, Sxx = sum i i m, Sxy = sum i j m, Sxz, Syy,
 *     Syz, Szz
 *   data sums in binary64, per component c of u, v, w, with t = (double)d_c at a present point and +0 elsewhere, formed separably
 *     x, then y, then z; every sum as (((t[-r] + t[-r+1]) + ...) + t[r]) in ascending offset, every addition and every product by the
 *     (double) integer offset rounded on its own, no running add / subtract sums (the discipline of f3d_local_correlation):
 *       along x:  a0 = sum t,     a1 = sum (i * t)
 *       along y:  b00 = sum a0,   b10 = sum a1,    b01 = sum (j * a0)
 *       along z:  D0 = sum b00,   Dx = sum b10,    Dy = sum b01,   Dz = sum (k * b00)
 *   normal matrix, exact integers:  C_ab = n S_ab - S_a S_b (symmetric 3 x 3); for an axis of size 1 C_aa = 1 (its off-diagonals and
 *     right-hand side are 0 by themselves, so its column of G comes out 0, as in f3d_flow_strain).  adj = adjugate of C, and
 *     det = C_00 adj_00 + C_01 adj_10 + C_02 adj_20 in int64.  |C| < 2^19, |adj| < 2^39 and det < 2^57 at radius <= 3; at radius 4
 *     det leaves int64, so radius is 1 .. 3.
 *   right-hand side and solution in binary64:  r_a = n * D_a - S_a * D0 (integers converted exactly),
 *     num_a = (adj_a0 * r_0 + adj_a1 * r_1) + adj_a2 * r_2,  G[c][a] = (float)(num_a / (double)det): one IEEE binary64 division per
 *     entry, nothing else in binary64 but + - *.
 *   undefined voxel (every selected output NaN):  p absent (lost);  else n < min_count or det == 0, which is exact: the present
 *     points are coplanar (thin).
 * Outputs, in this order (out[0..16]), selected by group:
 *   F3D_STRAIN_VOL  out[0] vol;  F3D_STRAIN_E  out[1..6] exx eyy ezz exy exz eyz;  F3D_STRAIN_EQ  out[7] eq: from this G by exactly
 *                   the float32 expressions of f3d_flow_strain
 *   F3D_WSTRAIN_G   out[8..16] G00 G01 G02 G10 G11 G12 G20 G21 G22 (row = component u v w, column = axis x y z)
 * Geometry from the current container (f3d_set_container), whole volume, library stream.  Entries of out for groups not selected
 * are ignored and never written.  Refused: a null input; a null selected output; fields 0 or with unknown bits; a selected output
 * that is also an input; two selected outputs that are the same container; radius outside 1 .. 3; min_count outside
 * 1 .. (2 radius + 1)^3; an empty or too large size.
 * stats (nullable; asking waits for the stream): defined, folded, vol_min, vol_max, eq_max, vol_sum as in f3d_strain_stats, lost and
 * thin as above.  vol and eq are computed for the statistics whether or not they are stored. */
#define F3D_WSTRAIN_G 8u
typedef struct f3d_window_strain_stats {
  unsigned long long defined, folded, lost, thin;
  float vol_min, vol_max, eq_max;
  double vol_sum;
} f3d_window_strain_stats;
int f3d_window_strain(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[17], unsigned fields, unsigned radius,
                      unsigned min_count, size_t width, size_t height, size_t depth,
                      f3d_window_strain_stats* stats /* nullable; non-null waits */);

/* Principal strains of a displacement: the eigenvalues e1 >= e2 >= e3 of the Green-Lagrange tensor E of f3d_flow_strain (largest
 * extension, largest compaction, independent of how the sample sits in the grid), the maximum shear and the directions of e1 and
 * e3, in one stencil pass from d = (u, v, w); E itself is not stored.  Per voxel:
 * 1. G, the missing-sample rules and the set of undefined voxels are exactly f3d_flow_strain's, and E (Exx Eyy Ezz Exy Exz Eyz) is
 *    formed from G by exactly its expressions, so the tensor diagonalised here is the one f3d_flow_strain stores.  An undefined
 *    voxel is NaN in every output.
 * 2. Cyclic Jacobi: A = E (a00 a11 a22 a01 a02 a12, symmetric), V = I.  Five sweeps; in each sweep the pairs
 *    (p, q) = (0,1), (0,2), (1,2) in this order, r the third index.  For a pair, every operation float32, rounded on its own, in
 *    exactly this order (only + - * / and sqrt: float32 numpy agrees bit for bit, which the closed trigonometric form would not):
 *      if a_pq == 0: nothing happens               (so a sweep that finds all three off-diagonals zero is the identity)
 *      theta = (a_qq - a_pp) / (2.f * a_pq)
 *      t = 1.f / (fabsf(theta) + sqrtf(theta * theta + 1.f)) ;  if theta < 0: t = -t
 *      c = 1.f / sqrtf(t * t + 1.f) ;  s = t * c ;  h = t * a_pq
 *      a_pp = a_pp - h ;  a_qq = a_qq + h ;  a_pq = 0.f
 *      (a_rp, a_rq) = (c * a_rp - s * a_rq,  s * a_rp + c * a_rq)              (old values on the right)
 *      for k in 0..2:  (V_kp, V_kq) = (c * V_kp - s * V_kq,  s * V_kp + c * V_kq)
 *    Five sweeps leave no off-diagonal on any tensor tried; the count is fixed and part of the definition.
 * 3. lambda_i = a_ii, direction i = column i of V.  Ordered by three compare-exchanges (0,1), (0,2), (1,2): value and column are
 *    exchanged together when lambda_i < lambda_j (strictly, so equal values keep their order).  e1, e2, e3 = the three values;
 *    gmax = 0.5f * (e1 - e3).
 * 4. Sign of a stored direction d: k = the first of x, y, z with the largest fabsf(d_k); if d_k < 0 all three components are
 *    negated.  The middle direction is d3 x d1 and is not stored.
 * Outputs, in this order (out[0..9]), selected by group:
 *   F3D_PRINCIPAL_VALUES  out[0..2] e1 e2 e3
 *   F3D_PRINCIPAL_SHEAR   out[3]    gmax
 *   F3D_PRINCIPAL_DIR1    out[4..6] x, y, z components of the unit direction of e1
 *   F3D_PRINCIPAL_DIR3    out[7..9] x, y, z components of the unit direction of e3
 * Geometry from the current container (f3d_set_container), whole volume, library stream.  Entries of out for groups not selected
 * are ignored and never written.  Refused: a null input; a null selected output; fields 0 or with unknown bits; a selected output
 * that is also an input; two selected outputs that are the same container.
 * stats (nullable; asking waits for the stream): over the voxels whose e1 is not NaN, defined = their number, e1_max, e3_min and
 * shear_max = the exact max of e1, min of e3 and max of gmax (NaN when there is none), whether or not those fields are stored. */
#define F3D_PRINCIPAL_VALUES 1u
#define F3D_PRINCIPAL_SHEAR 2u
#define F3D_PRINCIPAL_DIR1 4u
#define F3D_PRINCIPAL_DIR3 8u
typedef struct f3d_principal_stats {
  unsigned long long defined;
  float e1_max, e3_min, shear_max;
} f3d_principal_stats;
int f3d_principal_strain(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[10], unsigned fields, size_t width,
                         size_t height, size_t depth, f3d_principal_stats* stats /* nullable; non-null waits */);

/* Polar decomposition F = R U of the local deformation gradient F = I + G of a displacement: the rotation of each material
 * neighbourhood (to which E = 1/2 (F^T F - I) is blind by construction) as an angle and a rotation vector, and the principal
 * stretches, in one stencil pass from d = (u, v, w); neither F nor R is stored.  Every operation float32, rounded on its own, in
 * exactly the order written; only + - * / and sqrt occur, so float32 numpy agrees bit for bit.  Per voxel:
 * 1. G, the missing-sample rules and the set of undefined voxels are exactly f3d_flow_strain's; vol and E (Exx Eyy Ezz Exy Exz Eyz)
 *    are formed from G by exactly its expressions.  An undefined voxel is NaN in every output.
 * 2. (A, V) = rule 2 of f3d_principal_strain unchanged: five cyclic Jacobi sweeps on A = E, V = I.
 * 3. m_i = 2.f * a_ii + 1.f (i = 0, 1, 2): the eigenvalues of C = F^T F.  The voxel is FOLDED when vol <= -1.f or !(m_i > 0.f) for
 *    any i: F has no rotation there (det R would be -1); a folded voxel is NaN in every output.  Otherwise lambda_i = sqrtf(m_i),
 *    and l1, l2, l3 = the three lambda ordered by the compare-exchanges (0,1), (0,2), (1,2) of f3d_principal_strain's rule 3 (values
 *    only, exchanged when strictly smaller).  Nothing below depends on that order.
 * 4. q_i = 1.f / lambda_i
 *    Uinv_rc = ((V_r0 * q_0) * V_c0 + (V_r1 * q_1) * V_c1) + (V_r2 * q_2) * V_c2            (all nine; r, c in {0,1,2})
 *    Fm = G with 1.f added to G00, G11 and G22
 *    R_rc = (Fm_r0 * Uinv_0c + Fm_r1 * Uinv_1c) + Fm_r2 * Uinv_2c
 * 5. c = 0.5f * (((R00 + R11) + R22) - 1.f)
 *    ax = 0.5f * (R21 - R12) ;  ay = 0.5f * (R02 - R20) ;  az = 0.5f * (R10 - R01)
 *    s = sqrtf((ax*ax + ay*ay) + az*az)
 *    theta = ATAN2(s, c)                                                                     (rule 6; 0 .. pi)
 *    k = theta / s ;  (rx, ry, rz) = (k * ax, k * ay, k * az) ;  if s == 0: (rx, ry, rz) = (0, 0, 0)
 *    The skew part of an exact half turn vanishes and gives no axis: there theta is pi and the rotation vector is 0.
 * 6. ATAN2(s, c) for s >= 0, with K3, K5, K7, K9 the float32 nearest to 1/3, 1/5, 1/7, 1/9 (0x3EAAAAAB, 0x3E4CCCCD, 0x3E124925,
 *    0x3DE38E39), PI_F = 0x40490FDB and HALFPI_F = 0x3FC90FDB:
 *      big = fabsf(c) >= s
 *      x = big ? s / c : c / s ;  if s == 0 and c == 0: x = 0.f
 *      twice:  x = x / (1.f + sqrtf(x * x + 1.f))                        (the tangent of half the angle; |x| <= tan(pi/16) after it)
 *      z = x * x
 *      p = (((z * K9 - K7) * z + K5) * z - K3) * z + 1.f
 *      t = 4.f * (x * p)
 *      theta = big ? (c > 0.f ? t : PI_F + t) : HALFPI_F - t
 * Outputs, in this order (out[0..6]), selected by group:
 *   F3D_POLAR_ANGLE    out[0]    theta: the rotation angle in radians
 *   F3D_POLAR_VECTOR   out[1..3] rx ry rz: the rotation vector theta * n, n the unit axis (right-handed, x y z components)
 *   F3D_POLAR_STRETCH  out[4..6] l1 >= l2 >= l3: the principal stretches (the eigenvalues of U; their logarithms are the Hencky strains)
 * Geometry from the current container (f3d_set_container), whole volume, library stream.  Entries of out for groups not selected
 * are ignored and never written.  Refused: a null input; a null selected output; fields 0 or with unknown bits; a selected output
 * that is also an input; two selected outputs that are the same container.
 * stats (nullable; asking waits for the stream): folded = the folded voxels; over the others that are defined: defined = their
 * number, theta_max, l1_max and l3_min = the exact max of theta, max of l1 and min of l3 (NaN when there is none), theta_sum = the sum
 * of theta in double in the fixed order of the reduction (0 when there is none) -- all whether or not those fields are stored. */
#define F3D_POLAR_ANGLE 1u
#define F3D_POLAR_VECTOR 2u
#define F3D_POLAR_STRETCH 4u
typedef struct f3d_polar_stats {
  unsigned long long defined, folded;
  float theta_max, l1_max, l3_min;
  double theta_sum;
} f3d_polar_stats;
int f3d_polar_decomposition(f3d_devptr u, f3d_devptr v, f3d_devptr w, const f3d_devptr out[7], unsigned fields, size_t width,
                            size_t height, size_t depth, f3d_polar_stats* stats /* nullable; non-null waits */);

/* Principal strains and the polar decomposition of a STORED displacement gradient: what f3d_principal_strain and
 * f3d_polar_decomposition compute, with G read from nine containers instead of formed by central differences -- the least-squares
 * gradient of f3d_window_strain (its F3D_WSTRAIN_G group, whose noise is a third to a twenty-fifth of the stencil's, so the
 * eigenvalues no longer repel), an FE solution, a filter of the caller's.  No new arithmetic; per voxel:
 *   grad[0..8] = G00 G01 G02 G10 G11 G12 G20 G21 G22 (F3D_WSTRAIN_G's order: row = component u v w, column = axis x y z), float
 *   containers of the current container geometry.  Two entries may be the same container.
 *   The voxel is UNDEFINED iff any of its nine entries is NaN; an undefined voxel is NaN in every output.  Otherwise the arithmetic
 *   runs as written (an infinity gives whatever the rules give): E from G by f3d_flow_strain's expressions (and vol, for the polar
 *   entry), then
 *     f3d_principal_from_gradient:  rules 2 - 4 of f3d_principal_strain, unchanged;
 *     f3d_polar_from_gradient:      rules 2 - 6 of f3d_polar_decomposition, unchanged, the folded rule (vol <= -1.f or
 *                                   !(m_i > 0.f)) included.
 * Output order, groups (F3D_PRINCIPAL_* / F3D_POLAR_*), the statistics and their reduction order are those of
 * f3d_principal_strain / f3d_polar_decomposition: the gradient f3d_flow_strain's rules give, with NaN at its undefined voxels, fed
 * to these entries gives the outputs and statistics of those two bit for bit, theta_sum included.
 * Geometry from the current container (f3d_set_container), whole volume, library stream.  Entries of out for groups not selected
 * are ignored and never written.  Refused: a null grad or a null entry of it; a null selected output; fields 0 or with unknown
 * bits; a selected output that is any of the nine inputs; two selected outputs that are the same container; an empty or too large
 * size.  stats: nullable; asking waits for the stream. */
int f3d_principal_from_gradient(const f3d_devptr grad[9], const f3d_devptr out[10], unsigned fields, size_t width, size_t height,
                                size_t depth, f3d_principal_stats* stats /* nullable; non-null waits */);
int f3d_polar_from_gradient(const f3d_devptr grad[9], const f3d_devptr out[7], unsigned fields, size_t width, size_t height,
                            size_t depth, f3d_polar_stats* stats /* nullable; non-null waits */);

/* Inverse displacement (no reference counterpart).  d = (d_u, d_v, d_w) is the displacement of every voxel of frame 0 on frame 0's
 * grid (a pair's flow, or f3d_compose_flow's cumulative displacement), voxel units.  g = (g_u, g_v, g_w) is the map in the other
 * direction on frame k's grid: g(y) = -d(y + g(y)), by the fixed-point iteration g <- -d(y + g) of each voxel on its own.  With g a
 * field of frame 0 is carried onto frame k (f3d_carry_field below).  Per voxel (x, y, z), every operation float32, rounded on its own:
 *   S(g):  p = (x + g_u, y + g_v, z + g_w)                              (one float add per axis)
 *          p NaN, or outside [0, width-1] x [0, height-1] x [0, depth-1]:  the voxel is lost
 *          else s = d sampled trilinearly at p with f3d_compose_flow's expression tree: i = floorf(p), fractions f = p - i, upper
 *          corners min(n - 1, i + 1); per component, with c the eight corner values (x fastest),
 *            v0 = (1-fx)*(1-fy)*c000 + fx*(1-fy)*c100 + (1-fx)*fy*c010 + fx*fy*c110       (products and sums left to right)
 *            v1 = the same on the plane z1;   s = (1-fz)*v0 + fz*v1
 *          a NaN in any component of s:  the voxel is lost
 *   g_0 = (+0, +0, +0).  For n = 0, 1, ...:
 *          s = S(g_n);  e_c = g_n,c + s_c per component;  e = fmaxf(fmaxf(fabsf(e_u), fabsf(e_v)), fabsf(e_w))
 *          e <= tolerance or n == iterations:  the voxel stops with g = g_n and err = e
 *          else g_n+1 = -s  (the sign flipped per component)
 *   A voxel that is lost at any step is NaN in g_u, g_v, g_w and err.
 * So err is exactly the distance by which the round trip through the stored g misses, n is the number of steps taken, and a voxel
 * costs n + 1 samples.  Stopping per voxel is part of the definition: on smooth fields a few per cent of the voxels never reach a
 * bitwise fixed point but alternate between two values one ulp apart.  The iteration converges where the gradient of d is below 1 in
 * norm; elsewhere err and stats->unconverged say so.  No damping, no Newton step.
 * err is nullable.  Geometry from the current container (f3d_set_container), whole volume, library stream.  Refused (status 1, a
 * message, nothing written): a null input or g output; an output that is also an input; two outputs that are the same container;
 * iterations outside 1 .. 64; tolerance NaN or negative.
 * stats (nullable; asking waits for the stream): defined = voxels whose g_u is not NaN, unconverged = defined voxels with
 * err > tolerance, steps_sum = the sum of n over the defined voxels (exact), err_max = the exact max of err over them (NaN when none
 * is defined).  The same numbers every run: per-workgroup partials folded in a fixed order, no float atomics. */
typedef struct f3d_inverse_stats {
  unsigned long long defined, unconverged, steps_sum;
  float err_max;
} f3d_inverse_stats;
int f3d_invert_displacement(f3d_devptr d_u, f3d_devptr d_v, f3d_devptr d_w, f3d_devptr g_u, f3d_devptr g_v, f3d_devptr g_w,
                            f3d_devptr err /* nullable */, size_t width, size_t height, size_t depth, unsigned iterations,
                            float tolerance, f3d_inverse_stats* stats /* nullable; non-null waits */);

/* A field gathered through a displacement: out(x) = field(x + m(x)).  With m = g of f3d_invert_displacement it carries a field of
 * frame 0 (a strain field, labels) onto frame k's grid; with m = d it brings a field of frame k (the frame itself) back onto frame
 * 0's grid.  Unlike f3d_warp, a point outside the volume has a defined answer: NaN.  Per voxel:
 *   p = (x + m_u, y + m_v, z + m_w); p NaN or outside the volume (the test of S above):  out = NaN
 *   F3D_CARRY_LINEAR   the trilinear expression of S above on field (a NaN corner gives NaN)
 *   F3D_CARRY_NEAREST  the voxel at (int)floorf(p_c + 0.5f) per axis, clamped to n - 1, copied bit for bit (integer labels kept as
 *                      floats survive)
 * Geometry from the current container, whole volume, library stream.  Refused: a null argument; an unknown mode; out equal to an
 * input.  lost (nullable): the number of NaN outputs; asking for it waits for the stream, passing NULL does not. */
#define F3D_CARRY_LINEAR 1u
#define F3D_CARRY_NEAREST 2u
int f3d_carry_field(f3d_devptr field, f3d_devptr m_u, f3d_devptr m_v, f3d_devptr m_w, f3d_devptr out, size_t width, size_t height,
                    size_t depth, unsigned mode, unsigned long long* lost /* nullable; non-null waits */);

/* Per-voxel match quality of two volumes on one grid (no reference counterpart: the correlation coefficient a volume-correlation
 * workflow writes beside its displacement).  a and b are any two volumes; in practice a is frame 0 and b is frame 1 carried onto
 * frame 0's grid by f3d_carry_field, NaN where the point left the volume.  For every voxel, over the (2r+1)^3 window round it, the
 * zero-normalised cross-correlation (zncc) and the RMS difference (rmsd) of the voxels present in both.
 * Presence: a voxel is present when it is inside the volume and neither a nor b is NaN there.
 * Quantities per voxel, binary64:  m = 1 if present, else 0;  A = (double)a if present, else +0;  B likewise from b;
 *   q1 = m   q2 = A   q3 = B   q4 = A*A   q5 = B*B   q6 = A*B   q7 = (A - B)*(A - B)        (the difference taken in binary64)
 * Window sums, separably in the order x, then y, then z:
 *   X_j(x,y,z) = (((t_-r + t_-r+1) + ...) + t_r)  with t_i = q_j(x+i, y, z);  terms outside the volume are +0 addends
 *   Y_j = the same sum over X_j along y;  Z_j = the same sum over Y_j along z
 * Every addition is rounded on its own in binary64, in ascending order of the coordinate; there are no running add / subtract sums,
 * so a voxel's result does not depend on where a march started.  n, Sa, Sb, Saa, Sbb, Sab, Sdd = Z_1 .. Z_7.
 * Outputs, float32:
 *   the centre voxel absent:  both outputs NaN (the voxel counts as lost)
 *   rmsd = sqrtf((float)Sdd / (float)n)
 *   va = n*Saa - Sa*Sa ;  vb = n*Sbb - Sb*Sb ;  c = n*Sab - Sa*Sb        (binary64, every operation rounded on its own; no binary64
 *                                                                          division or square root anywhere)
 *   the window is flat when !(va > 0x1p-40 * (n*Saa)) or !(vb > 0x1p-40 * (n*Sbb))  (so a NaN counts as flat):  zncc = NaN
 *     (the rounding noise of the sums is a few 1e-16 relative: constant volumes stay below 5e-16, 2^-40 is 9.1e-13, and a volume
 *      of 1000 +- 0.01 is not flat)
 *   else zncc = (float)c / (sqrtf((float)va) * sqrtf((float)vb))        (float32 operations rounded on their own, IEEE / and sqrt)
 *   There is no clamp: a value may exceed 1 by an ulp.
 * Outputs selected by bit: F3D_CORRELATION_ZNCC out[0], F3D_CORRELATION_RMSD out[1].  Geometry from the current container
 * (f3d_set_container), whole volume, library stream.  Entries of out that are not selected are ignored and never written.  Refused:
 * a null input; a null selected output; fields 0 or with unknown bits; radius outside 1 .. 4; a selected output that is also an
 * input; two selected outputs that are the same container; a NaN threshold.  a and b may be the same container.
 * stats (nullable; asking waits for the stream): defined = voxels whose zncc is not NaN, lost = voxels whose centre is absent,
 * below = defined voxels with zncc < threshold, zncc_min = the exact min over the defined voxels (NaN when there is none), zncc_sum
 * accumulated in double over them (0 when none), rmsd_max = the exact max of rmsd over the voxels that are not lost (NaN when all
 * are).  The voxels that are neither defined nor lost are the flat ones.  Both outputs are computed for the statistics whether or
 * not they are stored.  The same numbers every run: per-workgroup partials folded in a fixed order, no float atomics. */
#define F3D_CORRELATION_ZNCC 1u
#define F3D_CORRELATION_RMSD 2u
typedef struct f3d_correlation_stats {
  unsigned long long defined, lost, below;
  float zncc_min, rmsd_max;
  double zncc_sum;
} f3d_correlation_stats;
int f3d_local_correlation(f3d_devptr a, f3d_devptr b, const f3d_devptr out[2], unsigned fields, unsigned radius, float threshold,
                          size_t width, size_t height, size_t depth, f3d_correlation_stats* stats /* nullable; non-null waits */);

/* Rigid-body or affine motion of a displacement (no reference counterpart: the drift, settling and tilt of a sample between two scans,
 * which a volume-correlation workflow takes out of a displacement before it looks at it).  Two device passes with a host solve
 * between them (f3d_motion_solve of include/f3d_host.h): the moment sums of d = (u, v, w), and the subtraction of a fit
 * d_fit(x) = t + M (x - centre).
 *
 * f3d_motion_sums.  A voxel is present when it is inside the volume, none of u, v, w is NaN there and, when weight is not 0,
 * weight[i] >= weight_min (a NaN weight fails the comparison and is absent; the mask is binary, there are no fractional weights).
 * centre c = ((width-1)/2, (height-1)/2, (depth-1)/2); X = x - c is a half-integer per axis, exact in binary64.  Over the present
 * voxels:
 *   n                  their number
 *   Sx[3]   = sum X                     Sxx[6] = sum X X^T in the order xx yy zz xy xz yz
 *   Sd[3]   = sum d                     Sxd[9] = sum X_i d_j, row i = coordinate, column j = component (Sxd[3*i + j])
 *   Sdd[3]  = sum d_j^2
 * n, Sx and Sxx are integer sums of the doubled coordinates 2x - (width-1) in signed 64 bits, converted at the end (one multiplication
 * by 0.5 or 0.25 of the integer rounded to binary64: exact whenever the sum is below 2^53).  The 64 bits hold for every volume of at
 * most 32768 along an axis and 2^33 voxels; larger ones are refused.
 * The d-sums are binary64 + and * only (no fma), d converted from float32, every operation rounded on its own:
 *   a lane owns the run of at most 32 planes [32 k, 32 k + 32) of one column (x, y) and adds its present voxels in ascending z from +0:
 *     s_j += d_j ;  sz_j += Z * d_j ;  q_j += d_j * d_j                       (j = u, v, w; the square of a float32 is exact)
 *   the column's constant X and Y are factored out of the run:  Sd_j gets s_j, Sxd_xj gets X * s_j, Sxd_yj gets Y * s_j, Sxd_zj gets sz_j,
 *   Sdd_j gets q_j  (so X * sum_z d, not sum_z X * d: one rounding of the product per run instead of one per voxel)
 *   then the fixed order of the statistics of the other entries: the xor butterfly 32, 16, ..., 1 over the 64 consecutive x of a wave, the
 *   4 rows of a workgroup in sequence, and the fold of the workgroup partials (x fastest, then y, then z): thread t takes t, t + 256, ...
 *   in that order, then the halving tree 128 ... 1.  A sum that is zero is +0.
 * The same input gives the same bytes every run (no float atomics).  Geometry from the current container (f3d_set_container), whole
 * volume, library stream; the call waits for the stream.  Refused (status 1, a message): a null u, v, w or out; a NaN weight_min when
 * weight is given; an empty or too large size.
 * (The struct is declared without a typedef because the entry has its name: write `struct f3d_motion_sums`.) */
struct f3d_motion_sums {
  unsigned long long n;
  double Sx[3], Sxx[6], Sd[3], Sxd[9], Sdd[3];
};
int f3d_motion_sums(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr weight /* 0: none */, float weight_min, size_t width,
                    size_t height, size_t depth, struct f3d_motion_sums* out);

/* f3d_remove_motion.  fit means d_fit(x) = t + M (x - centre), M row-major (M[3*r + c]: component r, coordinate c); only centre, t and
 * M are read here, the rest is what f3d_motion_solve reports: model (F3D_MOTION_*), n and rms_before = sqrt((Sdd_u + Sdd_v + Sdd_w) / n)
 * of the sums, and for the rigid model cos_angle = (tr R - 1) / 2 and the axial vector (R32 - R23, R13 - R31, R21 - R12) / 2 of
 * R = I + M (its length is the sine of the angle, its direction the axis); both are 0 for the other models.
 * Per voxel (x, y, z) and component r, with X = (double)x - centre[0], Y and Z likewise, in binary64, every operation rounded on its own,
 * in exactly this order (part of the ABI):
 *   res_r = (float)((double)d_r - (t_r + ((M_r0 * X + M_r1 * Y) + M_r2 * Z)))
 * NaN in, NaN out (per component).  In place (out_u == u, out_v == v, out_w == w) is allowed; any other aliasing between the six
 * volumes is refused, and so are a null volume or fit, a non-finite entry of centre, t or M, and an empty size; a refused call writes
 * nothing.  Geometry from the current container, whole volume, library stream.
 * stats (nullable; asking waits for the stream), from the stored float32 residuals: present = voxels none of whose three residuals is
 * NaN, sum_sq = the binary64 sum over them of (double)res_r * (double)res_r, added u, v, w per voxel along the lane's run and then in the
 * fixed order above, max_abs = the exact max of |res_r| over them (NaN when there is none). */
#define F3D_MOTION_TRANSLATION 0
#define F3D_MOTION_RIGID 1
#define F3D_MOTION_AFFINE 2
typedef struct f3d_motion_fit {
  double centre[3], t[3], M[9];
  unsigned long long n;
  double rms_before;
  double cos_angle, axial[3];
  int model;
} f3d_motion_fit;
typedef struct f3d_motion_residual {
  unsigned long long present;
  double sum_sq;
  float max_abs;
} f3d_motion_residual;
int f3d_remove_motion(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr out_u, f3d_devptr out_v, f3d_devptr out_w,
                      const f3d_motion_fit* fit, size_t width, size_t height, size_t depth,
                      f3d_motion_residual* stats /* nullable; non-null waits */);

/* Per-label motion of a displacement (no reference counterpart: the samples of in-situ tomography are mostly many bodies -- grains,
 * fibres, particles -- and what is asked of them is a table per body: how far it moved, how far it turned, how well a rigid motion
 * explains its voxels).  A segmentation is a container like every other (same pitch, 4 bytes per voxel) whose voxels are read as
 * int32; no float instruction touches them.  Label 0 is background, label L in 1 .. n_labels is body L, every other value (negative or
 * above n_labels) is foreign and ignored.  Two device passes with a host solve between them (f3d_motion_solve_labels of
 * include/f3d_host.h), as for the whole volume above.
 *
 * f3d_label_motion_sums.  out[L-1] receives the moment sums of label L about the centre of the volume.  A voxel takes part when it is
 * inside the volume, its label is in 1 .. n_labels, none of u, v, w is NaN there, weight[i] >= weight_min when weight is not 0 (a NaN
 * weight fails), and |d_j| < 1024 for every component.  info (nullable) counts every voxel of the volume exactly once, in this order:
 *   background     its label is 0
 *   foreign        its label is outside 0 .. n_labels
 *   absent         its label is in range, but a component is NaN or the weight fails
 *   out_of_range   it passes the above, but some |d_j| >= 1024 (an infinity included)
 *   used           it takes part
 * The sums are exact integers, so they depend on no summation order and the device adds them with integer atomics:
 *   q_j = (int)rintf(d_j * 16384.0f)     the product is exact (a power of two, no overflow; a denormal gives 0 either way), the rounding
 *                                        is to nearest, ties to even; |q_j| <= 2^24
 *   x2  = the doubled coordinates (2x - (width-1), 2y - (height-1), 2z - (depth-1)), as in f3d_motion_sums
 * and over the voxels of a label that take part
 *   n,  sum x2_i,  sum x2_i x2_k  (xx yy zz xy xz yz)             as in f3d_motion_sums
 *   Id_j = sum q_j      Ixd_ij = sum x2_i q_j      Idd_j = sum q_j^2
 * Each integer is rounded to binary64 once, to nearest even, and then scaled by a power of two (exact):
 *   Sx = 0.5 sum x2      Sxx = 0.25 sum x2 x2      Sd_j = 2^-14 Id_j      Sxd_ij = 2^-15 Ixd_ij  (Sxd[3*i + j])      Sdd_j = 2^-28 Idd_j
 * so Sd, Sxd and Sdd are the sums of the displacement quantised to 2^-14 voxel.  A label with no voxel gives all zeros (+0).
 * Widths: over one 64 x 4 x 32 tile (2^13 voxels) every sum fits signed 64 bits (q^2 < 2^48, |x2 q| < 2^40); over a label it does not
 * (Idd reaches 2^81), so the fifteen displacement sums are carried across tiles in two signed 64-bit limbs: a value v adds
 * v & 0xffffffff to lo and v >> 32 (arithmetic shift) to hi, and the total is hi 2^32 + lo as a 128-bit integer on the host (lo only
 * receives addends in [0, 2^32), at most 2^32 of them per label, and is read as unsigned).  The ten
 * coordinate sums are single 64-bit words under the size limits of f3d_motion_sums, which hold here too.
 * n_labels is 1 .. 2^22 (the accumulator is 320 B per label in a grow-only buffer of the library's, cleared on the stream before the
 * kernel and copied down after it).  Geometry from the current container, whole volume, library stream; the call waits for the
 * stream.  Refused (status 1, a message, nothing written): a null u, v, w, labels or out; n_labels 0 or above 2^22; a NaN weight_min
 * when weight is given; an empty or too large size. */
typedef struct f3d_label_info {
  unsigned long long background, foreign, absent, out_of_range, used;
} f3d_label_info;
int f3d_label_motion_sums(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr labels, size_t n_labels,
                          f3d_devptr weight /* 0: none */, float weight_min, size_t width, size_t height, size_t depth,
                          struct f3d_motion_sums* out /* n_labels entries, host */, f3d_label_info* info /* nullable */);

/* f3d_remove_label_motion.  fits and status are host arrays of n_labels entries, what f3d_motion_solve_labels wrote: the fit of label L
 * is fits[L-1] and is used when status[L-1] is F3D_LABEL_OK.  Per voxel (x, y, z) of label L and component r, with
 * X = (double)x - centre_L[0], Y and Z likewise, in binary64, every operation rounded on its own, in f3d_remove_motion's order:
 *   res_r = (float)((double)d_r - (t_r + ((M_r0 * X + M_r1 * Y) + M_r2 * Z)))
 * All three outputs are NaN where the label is background or foreign and where the label's status is not F3D_LABEL_OK; NaN in, NaN out
 * (per component).  In place (out_u == u, out_v == v, out_w == w) is allowed; any other aliasing between the six volumes, and the
 * label container among them, is refused, and so are a null volume, fits or status, n_labels 0 or above 2^22, a non-finite entry of
 * centre, t or M in a fit whose status is F3D_LABEL_OK, and an empty size; a refused call writes nothing.  The library uploads the
 * table of the fits per call and waits for that copy.  stats (nullable; asking waits for the stream) are f3d_remove_motion's, of the
 * stored residuals of the whole volume in the same fixed order.  The rms of one label's residual is sqrt((Sdd_u + Sdd_v + Sdd_w) / n)
 * of f3d_label_motion_sums of the residual.  Geometry from the current container, whole volume, library stream. */
#define F3D_LABEL_OK 0         /* fitted                                                              */
#define F3D_LABEL_EMPTY 1      /* no voxel took part                                                  */
#define F3D_LABEL_SMALL 2      /* fewer voxels than min_voxels                                        */
#define F3D_LABEL_DEGENERATE 3 /* the model is not determined (f3d_motion_solve refuses these sums)   */
int f3d_remove_label_motion(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr labels, size_t n_labels,
                            const f3d_motion_fit* fits, const int* status /* n_labels each, host */, f3d_devptr out_u,
                            f3d_devptr out_v, f3d_devptr out_w, size_t width, size_t height, size_t depth,
                            f3d_motion_residual* stats /* nullable; non-null waits */);

/* Contacts between labelled bodies (no reference counterpart: what is asked next of a granular or fibrous sample once every body has
 * its own motion -- which bodies touch, over what area and with which normal, and whether the contact opened, closed or slid).  The
 * volume is width x height x depth; the labels are a container read as int32 under the rules of f3d_label_motion_sums: 0 is background,
 * 1 .. n_labels are bodies, every other value is foreign.
 *
 * Faces.  A face is a pair of voxels p and p + e_k (k = x, y, z) that both lie inside the volume; there are
 * (W-1)HD + W(H-1)D + WH(D-1) of them.  Every face falls into exactly one class, decided in this order:
 *   foreign      either label is foreign
 *   background   both labels are 0
 *   surface      exactly one label is 0
 *   interior     the labels are equal
 *   contact      anything else: two different bodies
 * The contact of a contact face is the unordered pair (lo, hi), lo < hi, of its labels.  Its sign is s = +1 when label(p) == lo, so
 * that going along +k leads from lo into hi, and s = -1 otherwise.
 *
 * Sums of a contact, all exact 64-bit integers:
 *   faces[k]   the number of its faces along axis k
 *   area[k]    the sum of s over its faces along axis k: by the divergence theorem the area vector of the staircase patch, pointing
 *              from lo to hi (which is why it is kept signed)
 *   c2[j]      the sum over its faces of the doubled coordinate j of the face centre about the volume centre: for a face along k at
 *              p = (x_0, x_1, x_2) that is 2 x_k + 1 - (N_k - 1) for j == k and 2 x_j - (N_j - 1) for the other two
 *   n_jump, J  only when u, v and w are given (otherwise 0).  A contact face takes part when none of u, v, w is NaN and all are below
 *              1024 in magnitude at BOTH voxels; with q_j = (int)rintf(d_j * 16384.0f) as in f3d_label_motion_sums,
 *              J[j] = sum s * (q_j(p + e_k) - q_j(p)), the displacement of hi minus that of lo in units of 2^-14 voxel, and n_jump
 *              counts the faces that took part.
 * Widths: with at most 32768 voxels along an axis and 2^33 in all, a contact has fewer than 2^35 faces; a jump term is below 2^25 in
 * magnitude and a c2 term below 2^16, so every sum stays below 2^60 and single words suffice.
 *
 * f3d_contact_info counts every face exactly once in foreign, background, surface, interior, contact, and besides
 *   jump_absent  contact faces that did not take part in n_jump and J (all of them when u, v, w are not given)
 *   lost         contact faces that found no slot in the table (see below)
 *   n_contacts   occupied slots of the table: the number of distinct contacts when lost == 0, a lower bound otherwise
 *   complete     1 when lost == 0 and n_contacts <= capacity, else 0
 *
 * The key set is not known in advance, so the device keeps an open-addressed table in a grow-only buffer of the library's: the
 * smallest power of two of at least 2 * capacity slots of 112 B (the key (lo << 32) | hi and the 13 sums), cleared on the stream, a
 * slot claimed by a 64-bit compare-and-swap within at most 256 linear probes, the sums added with integer atomics.  Any schedule gives
 * the same sums.  When complete, out receives n_contacts entries sorted by (lo, hi) ascending: the same bytes on every call.  When not
 * -- more distinct contacts than capacity, or a face lost -- NOTHING is written to out (which faces are lost depends on the schedule),
 * the five class counters and jump_absent are still exact, the call returns 0 and the caller retries with more room.
 * Refused (status 1, a message, nothing written): a null labels, out or info; only some of u, v, w given; n_labels outside 1 .. 2^22;
 * capacity outside 1 .. 2^24; an empty volume or one above 32768 along an axis or 2^33 voxels; the label container among u, v, w.
 * Geometry from the current container, whole volume, library stream; the call waits for the stream. */
struct f3d_contact {
  int lo, hi;
  unsigned long long faces[3];
  long long area[3];
  long long c2[3];
  unsigned long long n_jump;
  long long J[3];
};
typedef struct f3d_contact_info {
  unsigned long long foreign, background, surface, interior, contact;
  unsigned long long jump_absent, lost, n_contacts;
  int complete;
} f3d_contact_info;
int f3d_label_contacts(f3d_devptr u, f3d_devptr v, f3d_devptr w /* all three or none (0) */, f3d_devptr labels, size_t n_labels,
                       size_t width, size_t height, size_t depth, size_t capacity,
                       struct f3d_contact* out /* capacity entries, host */, f3d_contact_info* info);

/* Connected bodies of a thresholded volume (no reference counterpart: f3d_label_motion_sums and f3d_label_contacts start from a label
 * volume, and a tomography user has grey values; this makes the labels where the frame already is).  The box is width x height x depth
 * in the corner of the current container; src is a container of floats, labels_out a container read as int32 under the convention of
 * f3d_label_motion_sums.  With W = width and H = height, the linear box index of the voxel (x, y, z) is x + W (y + H z).
 *
 * Foreground.  A voxel with value s is foreground when lo <= s && s <= hi in float compares.  A NaN voxel is therefore background, and
 * it is counted in nan.  lo may be -inf and hi +inf (an infinite voxel is then foreground); -0.0f equals 0.0f; a denormal compares as
 * its value.
 * Connectivity.  Six neighbours: two voxels are connected when they share a face, the faces of f3d_label_contacts.  Voxels that share
 * only an edge or a corner are not connected.
 * Component.  A maximal face-connected set of foreground voxels.  Its root is the smallest linear box index among its voxels, its size
 * is its voxel count.
 * Kept and dropped.  A component is kept when its size is at least min_voxels (at least 1).  The kept components are numbered
 * 1 .. n_labels in ascending order of root.  Every voxel of a kept component receives its number; every other voxel of the box receives
 * 0.  Container padding is neither read nor written, and no float instruction touches a label.
 * Sizes.  sizes[L - 1] is the size of label L, for L up to the smaller of n_labels and capacity; what lies beyond is not written.
 * f3d_component_info:
 *   foreground, background   every voxel of the box lies in exactly one of them
 *   nan                      the NaN voxels, which are contained in background
 *   n_components             kept and dropped components together
 *   n_labels                 kept components; dropped_components = n_components - n_labels
 *   dropped_voxels           the voxels of the dropped components; foreground - dropped_voxels voxels carry a label
 *   largest                  the size of the largest component, kept or not (0 without foreground)
 * Determinism.  Everything is a function of the input alone: two calls give the same bytes, whatever the schedule.
 * Limits.  At most 32768 voxels along an axis and 2^31 - 1 in the box, because a parent index is one 32-bit word (1024^3 is inside).
 * n_labels is not capped here; f3d_label_motion_sums and f3d_label_contacts keep their own limit of 2^22 labels.
 * Scratch: a grow-only buffer of the library's, 8 B per voxel of the box, 20 B per 1024 voxels, and 4 B per size handed out.
 * Refused (status 1, a message, nothing written): a null src, labels_out or info; src == labels_out; a NaN lo or hi, or lo > hi;
 * min_voxels of 0; an empty box, or a box beyond the limits; a box larger than the current container; sizes given with capacity 0.
 * Library stream; the call waits until info and sizes are on the host. */
typedef struct f3d_component_info {
  unsigned long long foreground, background, nan;
  unsigned long long n_components, n_labels, dropped_components, dropped_voxels, largest;
} f3d_component_info;
int f3d_label_components(f3d_devptr src, float lo, float hi, unsigned long long min_voxels, f3d_devptr labels_out, size_t width,
                         size_t height, size_t depth, unsigned long long* sizes /* host, nullable */, size_t capacity,
                         f3d_component_info* info /* required */);

/* Exact squared Euclidean distance and nearest-seed (feature) transform (no reference counterpart: the primitive under a split of
 * touching bodies, and alone the depth of every voxel below a surface).  The box is width x height x depth in the corner of the current
 * container, the box index of the voxel (x, y, z) is x + W (y + H z) as for f3d_label_components, and seeds is a container read as int32
 * under the convention of f3d_label_motion_sums.
 *
 * Seeds.  mode F3D_SEED_NONZERO: the voxels of the box with value != 0.  F3D_SEED_ZERO: those with value == 0 (the classic distance
 * to the background of a label volume or mask).  Voxels outside the box do not exist: they are neither seeds nor background.
 * Nearest seed.  The squared distance of the voxels p and s is (px - sx)^2 + (py - sy)^2 + (pz - sz)^2, an integer.  The nearest
 * seed of p is the seed that minimises the pair (squared distance, box index) lexicographically: of several seeds at the same distance
 * the one with the smallest box index wins.  A seed is its own nearest seed at distance 0.
 * Outputs, each nullable, at least one required, each a container written inside the box only:
 *   d2_out     int32, the squared distance to the nearest seed.  With F3D_NEAREST_D2_FLOAT in flags it is stored as (float)d2 rounded
 *              to nearest even instead, so that it can be f3d_label_components' src; the conversion is monotone (a <= b gives
 *              (float)a <= (float)b), so thresholds on it select the same voxels up to the rounding of the bound, and exact below 2^24
 *   index_out  int32, the box index of the nearest seed
 *   value_out  int32, seeds[] at the nearest seed (0 in mode F3D_SEED_ZERO)
 * Without any seed in the box every voxel gets d2 = 2^31 - 1 (its float form with the flag), index = -1, value = 0.
 * f3d_nearest_info: seeds, the seeds in the box; d2_max, the largest stored d2 (2^31 - 1 without a seed); unreached, the voxels
 * without a nearest seed: the voxel count of the box when seeds == 0 and 0 otherwise.
 * Exactness and determinism.  No float instruction touches a distance; the float form of d2_out is one final conversion.  Every output
 * is a function of the input alone: two calls give the same bytes, whatever the schedule.
 * Limits.  At most 32768 voxels along an axis and 2^31 - 1 in the box, and in addition W^2 + H^2 + D^2 <= 2^31 - 1 so that every
 * distance fits (a cube of up to 26754 along the edge is inside; 32768 x 32768 x 1 is not).
 * Scratch: a grow-only buffer of the library's, 12 B per voxel of the box.  Container padding is neither read nor written.
 * Refused (status 1, a message, nothing written): a null seeds or info; no output selected; an output that is the container of seeds
 * or of another output; an unknown mode or flag; an empty box, a box beyond the limits, a box larger than the current container.
 * Library stream; the call waits until info is on the host. */
#define F3D_SEED_NONZERO 0u
#define F3D_SEED_ZERO 1u
#define F3D_NEAREST_D2_FLOAT 1u
typedef struct f3d_nearest_info {
  unsigned long long seeds, d2_max, unreached;
} f3d_nearest_info;
int f3d_nearest_seed(f3d_devptr seeds, unsigned mode, unsigned flags, f3d_devptr d2_out /* nullable */, f3d_devptr index_out /* nullable */,
                     f3d_devptr value_out /* nullable */, size_t width, size_t height, size_t depth, f3d_nearest_info* info /* required */);

/* Bodies of a thresholded volume with touching bodies taken apart (no reference counterpart: f3d_label_components joins everything
 * that shares a face, so a packed granular sample, a foam or a fibre mat is one component and has no contact; this splits it at its
 * necks).  Arguments, box, box index, foreground rule, sizes and capacity are f3d_label_components'; core_d2 >= 1 is added.
 *   1. F is the foreground: lo <= s && s <= hi, a NaN is background.
 *   2. C is the set of face-connected components of F, all of them.
 *   3. d2(p), p in F, is the squared distance to the nearest voxel of the box that is not in F: f3d_nearest_seed in mode F3D_SEED_ZERO
 *      on the mask, 2^31 - 1 when F is the whole box (voxels outside the box do not exist and are not background).
 *   4. The core voxels are those of F with d2 >= core_d2 (compared as 64-bit integers).  M is the set of face-connected components of
 *      the core mask, the core bodies.
 *   5. For p in F let s be the core voxel nearest to p in f3d_nearest_seed's order (squared distance, then box index), over ALL core
 *      voxels.  If there is none, or s lies in another component of C than p, p belongs to the remainder of its component; otherwise
 *      to the core body of s.
 *   6. The classes are the core bodies and, per component that has remainder voxels, its remainder.  The root of a class is the
 *      smallest box index among its voxels, its size their number.  The classes of at least min_voxels voxels are numbered
 *      1 .. n_labels in ascending order of root; every other voxel of the box receives 0.
 * Consequences.  With core_d2 = 1 every foreground voxel is a core voxel and its own nearest one, and labels_out, sizes and the first
 * eight counters equal f3d_label_components' byte for byte.  The assignment is Euclidean, not geodesic: a class need not be
 * face-connected, and a core body reaches exactly as far as its voxels are the nearest core voxels inside the component.
 * f3d_split_info: the eight fields of f3d_component_info with "component" read as class (n_components: kept and dropped classes,
 * largest: the largest class), and then
 *   connected_components   the components of C (f3d_label_components' n_components with min_voxels = 1)
 *   core_voxels, n_cores   the core voxels and the core bodies M
 *   remainder_bodies       the classes that are a remainder;  n_components = n_cores + remainder_bodies
 *   remainder_voxels       their voxels
 * Determinism and exactness as for the two entries it is made of: integers only, the same bytes on every call.
 * Limits: f3d_nearest_seed's.  Scratch: the library's grow-only buffer, 32 B per voxel of the box (4.3 GB at 512^3), 20 B per 1024
 * voxels and 4 B per size handed out.
 * Refused (status 1, a message, nothing written): what f3d_label_components refuses, core_d2 of 0, and a box whose squared diagonal
 * W^2 + H^2 + D^2 exceeds 2^31 - 1.  Library stream; the call waits until info and sizes are on the host. */
typedef struct f3d_split_info {
  unsigned long long foreground, background, nan;
  unsigned long long n_components, n_labels, dropped_components, dropped_voxels, largest;
  unsigned long long connected_components, core_voxels, n_cores, remainder_bodies, remainder_voxels;
} f3d_split_info;
int f3d_split_components(f3d_devptr src, float lo, float hi, unsigned long long core_d2, unsigned long long min_voxels,
                         f3d_devptr labels_out, size_t width, size_t height, size_t depth, unsigned long long* sizes /* host, nullable */,
                         size_t capacity, f3d_split_info* info /* required */);

/* Grey-value histogram and finite value range of a volume (no reference counterpart: what a user needs before f3d_label_components,
 * whose lo and hi have to come from somewhere, and the exact counts and ranks of any derived field).  The volume is width x height x
 * depth; src is a container of floats; mask is 0 for none, or a container read as int32: where it is 0 the voxel is masked, every
 * other value (a negative one too) lets it through.  Container padding is not read.
 *
 * The bin rule (csrc/f3d_histogram_bin.h, one text for the kernel and the host).  With lo < hi both finite, bins in 1 .. 4096 and
 * scale = (float)bins / (hi - lo) formed once in float32 on the host, a voxel value s takes part when lo <= s && s <= hi in float
 * compares; a NaN never takes part.  Its bin is min((int)((s - lo) * scale), bins - 1): the subtraction and the product are each
 * rounded to float32 (contraction is off) and the conversion truncates.  Each step is monotone in s, so every bin is an interval of
 * floats, and s == hi lands in the last bin.  -0.0f equals 0.0f; a denormal counts as its value.
 * f3d_histogram_info counts every voxel of the volume exactly once, tried in this order:
 *   masked   the mask is 0 there
 *   nan      s is a NaN
 *   below    s < lo (-inf included)
 *   above    s > hi (+inf included)
 *   used     the voxel is counted in counts[its bin]:  sum(counts) == used
 * f3d_value_range gives the smallest and the largest FINITE value of the voxels the mask lets through.  Values are compared by the
 * totally ordered integer key of their bits (sign-magnitude folded to an unsigned), so -0.0f is below +0.0f, a denormal keeps its value
 * and the result does not depend on the schedule.  f3d_range_info counts every voxel exactly once, in this order: masked, nan, infinite,
 * finite.  With finite == 0, min is +inf and max is -inf.
 * Determinism.  Counts and counters are integers added with integer atomics, min and max a maximum over integer keys: two calls give
 * the same bytes, whatever the schedule.  Workgroups count in LDS in 32-bit words (the lanes of a wave first merge their runs of equal
 * bins, so a constant row costs one add) and add what is non-zero to a 64-bit accumulator of `bins` words in a grow-only buffer of
 * the library's, cleared on the stream before the kernel.  No lane waits for another.
 * Limits: f3d_label_contacts'.  At most 32768 voxels along an axis and 2^33 in all.
 * Refused (status 1, a message, nothing written): a null src, counts, info, min or max; lo >= hi, a bound that is not finite, a hi - lo
 * or a scale that is not finite and positive in float32, bins outside 1 .. 4096; an empty volume, one beyond the limits or larger
 * than the current container.  Geometry from the current container, whole volume, library stream; the call waits for the stream. */
typedef struct f3d_histogram_info {
  unsigned long long masked, nan, below, above, used;
} f3d_histogram_info;
typedef struct f3d_range_info {
  unsigned long long masked, nan, infinite, finite;
} f3d_range_info;
int f3d_value_range(f3d_devptr src, f3d_devptr mask /* 0: none */, size_t width, size_t height, size_t depth, float* min, float* max,
                    f3d_range_info* info);
int f3d_histogram(f3d_devptr src, f3d_devptr mask /* 0: none */, float lo, float hi, size_t bins, size_t width, size_t height, size_t depth,
                  unsigned long long* counts /* bins entries, host */, f3d_histogram_info* info);

/* Shape sums of labelled bodies (no reference counterpart: what the shape table of a granular or fibrous study is made of -- size,
 * bounding box, axes, surface, whether a body is cut by the edge of the scan and whether it has a hole or a cavity).  The entry needs
 * the labels alone.  The box is width x height x depth (W x H x D = N_0 x N_1 x N_2) in the corner of the current container; labels is
 * a container read as int32 under the rules of f3d_label_motion_sums: 0 is background, 1 .. n_labels are bodies, every other value is
 * foreign.  Voxels outside the box do not exist: container padding is never read, as a voxel or as a neighbour, whatever it holds.
 *
 * out[L-1] receives 36 exact 64-bit integers of label L, over the voxels p = (x_0, x_1, x_2) of the box with label(p) == L, in plain
 * integer voxel coordinates:
 *   n            their number
 *   lo[3], hi[3] the smallest and the largest x_i among them; for a label without a voxel lo[i] = 0 and hi[i] = -1
 *   s1[3]        sum x_i
 *   s2[6]        sum x_i x_k in the order xx yy zz xy xz yz
 *   pairs[13]    for the direction d_k, the number of p with p and p + d_k in the box and label(p) == label(p + d_k) == L; d_k in this
 *                order: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,-1,0) (1,0,1) (1,0,-1) (0,1,1) (0,1,-1) (1,1,1) (1,1,-1) (1,-1,1) (1,-1,-1):
 *                one of each of the 13 pairs of opposite directions to the 26 neighbours
 *   squares[3]   the unit squares {p, p + e_i, p + e_k, p + e_i + e_k} in the planes xy, xz, yz with all four voxels in the box and of L
 *   cubes        the blocks p + {0,1}^3 with all eight voxels in the box and of L
 *   border[3]    per axis i, the sum of [x_i == 0] + [x_i == N_i - 1]: a voxel of a box one voxel thick along i counts twice
 * info (nullable) counts every voxel of the box exactly once: background (label 0), foreign (outside 0 .. n_labels) or labelled.
 * Determinism.  Everything is an integer function of the input, added with integer atomics: two calls give the same bytes, whatever
 * the schedule.
 * Limits: f3d_label_components'.  At most 32768 voxels along an axis and 2^31 - 1 in the box.  Widths: a term of s2 is below 2^30, so
 * s2 < 2^61; s1 < 2^46; every count is at most 2 * (2^31 - 1): single words suffice.  The device accumulates a lane's run over the 32
 * planes of a tile in 32-bit registers, a 64 x 4 x 32 tile (2^13 voxels) in LDS (s2 < 2^43 in 64-bit words, every other sum below
 * 2^28 in 32-bit words), the extents as maxima of x_i and of N_i - 1 - x_i so that cleared memory is their identity.
 * n_labels is 1 .. 2^22: the accumulator is 288 B per label in a grow-only buffer of the library's, cleared on the stream before the
 * kernel and copied down after it.
 * Refused (status 1, a message, nothing written): a null labels or out; n_labels outside 1 .. 2^22; an empty box, or a box beyond the
 * limits; a box larger than the current container.  Library stream; the call waits for the stream.
 * The solve from the sums to centroid, axes, surface, sphericity and Euler number is host code: f3d_label_shape_solve of
 * include/f3d_host.h. */
struct f3d_label_shape_sums {
  unsigned long long n;
  long long lo[3], hi[3];
  unsigned long long s1[3], s2[6];
  unsigned long long pairs[13], squares[3], cubes, border[3];
};
typedef struct f3d_label_shape_info {
  unsigned long long background, foreign, labelled;
} f3d_label_shape_info;
int f3d_label_shape_sums(f3d_devptr labels, size_t n_labels, size_t width, size_t height, size_t depth,
                         struct f3d_label_shape_sums* out /* n_labels entries, host */, f3d_label_shape_info* info /* nullable */);

/* Overlap of two labelled volumes through a displacement (no reference counterpart: which body of a later frame is which body of the
 * first one, which grain broke, which two sintered, which left the field of view -- and a check of the displacement that the grey values
 * do not see).  The volume is width x height x depth (W x H x D = N_0 x N_1 x N_2).  labels_a is a container read as int32 on the grid
 * of the displacement under the rules of f3d_label_motion_sums: 0 is background, 1 .. n_a are bodies, every other value is foreign.
 * labels_b is the same with n_b, on the grid the displacement leads to.  u, v, w are given all three or none (0): none is the identity.
 *
 * Classes.  Every voxel x = (x_0, x_1, x_2) of the volume falls into exactly one class, decided in this order:
 *   foreign_a        a = labels_a(x) is outside 0 .. n_a
 *   lost_background  p = x + d(x), one float32 add per axis ((float)x_0 + u(x), ...; with no u, v, w p = x), is NaN in a component or
 *   lost_body        outside [0, W-1] x [0, H-1] x [0, D-1] (the test of f3d_invert_displacement and f3d_carry_field): lost_background
 *                    when a == 0, lost_body otherwise
 *   foreign_b        y_c = min(N_c - 1, (int)floorf(p_c + 0.5f)) per axis, float32 add included (the rule of F3D_CARRY_NEAREST);
 *                    b = labels_b(y) is outside 0 .. n_b
 *   background       a == 0 and b == 0
 *   overlap          everything else
 * Keys.  An overlap voxel has the key (a, b): (a, 0) is the part of a body of A that landed on background, (0, b) the part of a body of
 * B that nothing of A reached.  A lost_body voxel has the key (a, -1), so that a body that partly left the volume shows it.  No other
 * voxel has a key.
 * Sums of a key, all exact 64-bit integers:
 *   n        its voxels
 *   ca2[j]   the sum of 2 x_j - (N_j - 1): the doubled source coordinates about the volume centre, as in f3d_label_contacts
 *   cb2[j]   the sum of 2 y_j - (N_j - 1); 0 for b == -1
 * so that (cb2 - ca2) / (2 n) is the exact mean displacement of the part, in whole voxels of B's grid, without any quantisation.
 * Widths: with at most 32768 voxels along an axis and 2^33 in all, a term is below 2^16 and every sum below 2^49.
 *
 * f3d_overlap_info counts every voxel exactly once in its first six fields, and besides
 *   table_lost   keyed voxels that found no slot in the table (see below)
 *   n_pairs      occupied slots of the table: the number of distinct keys when table_lost == 0, a lower bound otherwise
 *   complete     1 when table_lost == 0 and n_pairs <= capacity, else 0
 * The sum of n over the rows is lost_body + overlap.
 *
 * The table is f3d_label_contacts': an open-addressed table in a grow-only buffer of the library's, the smallest power of two of at
 * least 2 * capacity slots of 64 B (the key and the seven sums), cleared on the stream, a slot claimed by a 64-bit compare-and-swap
 * within at most 256 linear probes, the sums added with integer atomics.  Any schedule gives the same sums.  When complete, out
 * receives n_pairs entries sorted by (a, b) ascending as signed ints, so (a, -1) leads the rows of a: the same bytes on every call.
 * When not -- more distinct keys than capacity, or a voxel lost to the table -- NOTHING is written to out, the six class counters are
 * still exact, the call returns 0 and the caller retries with more room.
 * Refused (status 1, a message, nothing written): a null labels_a, labels_b, out or info; only some of u, v, w given; n_a or n_b
 * outside 1 .. 2^22; capacity outside 1 .. 2^24; an empty volume or one above 32768 along an axis or 2^33 voxels; labels_a and
 * labels_b being one container; a label container among u, v, w.  Container padding is never read.
 * Geometry from the current container, whole volume, library stream; the call waits for the stream.
 * The solve from the rows to matches, splits, merges and new numbers is host code: f3d_overlap_solve of include/f3d_host.h. */
struct f3d_overlap {
  int a, b;
  unsigned long long n;
  long long ca2[3], cb2[3];
};
typedef struct f3d_overlap_info {
  unsigned long long foreign_a, lost_background, lost_body, foreign_b, background, overlap;
  unsigned long long table_lost, n_pairs;
  int complete;
} f3d_overlap_info;
int f3d_label_overlap(f3d_devptr labels_a, size_t n_a, f3d_devptr labels_b, size_t n_b, f3d_devptr u, f3d_devptr v,
                      f3d_devptr w /* all three or none (0) */, size_t width, size_t height, size_t depth, size_t capacity,
                      struct f3d_overlap* out /* capacity entries, host */, f3d_overlap_info* info);

/* New numbers for the bodies of a label volume: out(x) = map[l - 1] for l = labels(x) in 1 .. n, 0 for l == 0 and 0 for a foreign l
 * (outside 0 .. n); the foreign voxels are counted in foreign (nullable; asking waits for the stream).  map is a host array of n ints,
 * none negative, uploaded per call into a grow-only buffer of the library's (the call waits for that copy); two labels may share a
 * number.  out may be labels itself: each voxel reads and writes its own word.  One streaming pass; container padding is neither read
 * nor written.  Refused (status 1, a message, nothing written): a null labels, map or out; n outside 1 .. 2^22; a negative map entry;
 * a volume above 32768 along an axis or one that does not fit the current container.  Geometry from the current container, whole
 * volume, library stream. */
int f3d_relabel_labels(f3d_devptr labels, size_t n, const int* map /* n entries, host */, f3d_devptr out, size_t width, size_t height,
                       size_t depth, unsigned long long* foreign /* nullable; non-null waits */);

/* Statistics of a scalar field per labelled body (no reference counterpart: what the equivalent strain, the volume change, the match
 * quality or the grey value say about every grain of a segmented sample, as exact sums that do not depend on the order).  The box is
 * width x height x depth in the corner of the current container; field is a container of floats; labels is a container read as int32
 * under the rules of f3d_label_motion_sums: 0 is background, 1 .. n_labels are bodies, every other value is foreign.  Container
 * padding is never read.
 *
 * Classes.  f3d_label_field_info (nullable) counts every voxel of the box exactly once, tried in this order, with s the field's value:
 *   background    the label is 0
 *   foreign       the label is outside 0 .. n_labels
 *   nan           s is a NaN
 *   out_of_range  t = s * scale, ONE float32 product with scale = ldexpf(1.0f, shift), has fabsf(t) > 16777216.0f: an infinity lands
 *                 here.  The product is exact unless it underflows, and then it is the float32 result of that product
 *   used          the voxel takes part:  sum of n over the rows == used
 * Quantisation.  A voxel that takes part has q = (int)rintf(t), to nearest, ties to even, so |q| <= 2^24 and every sum below is an
 * exact integer.  shift is -100 .. 100.
 * out[L-1] receives eight 64-bit words of label L, over the voxels of L that take part:
 *   n                  their number
 *   min_key, max_key   the smallest and the largest raw s among them as f3d_value_range's totally ordered integer key of the bits
 *                      (csrc/f3d_histogram_bin.h, key_of_bits): -0.0f is below +0.0f and a denormal keeps its value.  The key of a finite
 *                      float is never 0 or 0xffffffff; a label without a voxel gets min_key 0xffffffff and max_key 0
 *   iq                 sum q, signed; |iq| < 2^55
 *   iqq_lo, iqq_hi     sum q^2 (q^2 <= 2^48 and n < 2^31: below 2^79) in two limbs, the sum being hi * 2^32 + lo as a 128-bit integer.
 *                      On the device each addend v (a lane's run of at most 32 voxels, or the 2^13 voxels of a tile from the
 *                      workgroup's table: v < 2^61) adds v & 0xffffffff to lo and v >> 32 to hi, as f3d_label_motion_sums does;
 *                      neither limb overflows.  How the voxels fall into addends depends on the schedule, so the entry carries the
 *                      limbs before it writes out: iqq_lo is below 2^32 and iqq_hi is the rest, a function of the input alone
 *   below, above       with bins: the voxels with s < lo and with s > hi; 0 without
 * Bins.  bins is 0 .. 256.  With bins == 0, lo and hi are ignored, below = above = 0 and counts must be null.  With bins, lo < hi are
 * both finite, scale_b = (float)bins / (hi - lo) is formed as f3d_histogram forms it, and the bin rule of csrc/f3d_histogram_bin.h is
 * applied, unchanged, to the raw s of every voxel that takes part: s < lo adds to below, s > hi to above, every other voxel adds one to
 * counts[(L-1) * bins + min((int)((s - lo) * scale_b), bins - 1)].  So below + above + sum(counts row) == n for every label.
 * Determinism.  Everything is an integer function of the input, added with integer atomics, the extremes maxima over integer keys (the
 * device accumulates max(key) and max(0xffffffff - key), so that cleared memory is the identity): two calls give the same bytes.
 * Limits: f3d_label_shape_sums'.  At most 32768 voxels along an axis and 2^31 - 1 in the box; n_labels is 1 .. 2^22 and
 * n_labels * bins at most 2^26; counts are 32-bit.  The accumulators (64 B per label, the five counters, 4 B per count) live in a
 * grow-only buffer of the library's, cleared on the stream before the kernel and copied down after it.
 * Refused (status 1, a message, nothing written): a null field, labels or out; field and labels being one container; shift outside
 * -100 .. 100; bins above 256; counts given with bins == 0 or missing with bins > 0; what f3d_histogram refuses of lo, hi, bins;
 * n_labels outside 1 .. 2^22; n_labels * bins above 2^26; an empty box, a box beyond the limits or larger than the current
 * container.  Geometry from the current container, library stream; the call waits for the stream.
 * The solve from the rows to mean, deviation and quantiles is host code: f3d_label_field_solve of include/f3d_host.h. */
struct f3d_label_field_sums {
  unsigned long long n, min_key, max_key;
  long long iq;
  unsigned long long iqq_lo, iqq_hi, below, above;
};
typedef struct f3d_label_field_info {
  unsigned long long background, foreign, nan, out_of_range, used;
} f3d_label_field_info;
int f3d_label_field_sums(f3d_devptr field, f3d_devptr labels, size_t n_labels, int shift, float lo, float hi, size_t bins, size_t width,
                         size_t height, size_t depth, struct f3d_label_field_sums* out /* n_labels entries, host */,
                         unsigned* counts /* n_labels * bins entries, host; null iff bins == 0 */,
                         f3d_label_field_info* info /* nullable */);

/* A value per label painted into a volume: out(x) = values[l - 1] for l = labels(x) in 1 .. n_labels -- the bytes are copied, a NaN
 * keeps its payload -- and the quiet NaN 0x7fc00000 for background (0) and foreign (outside 0 .. n_labels) voxels.  values is a host
 * array of n_labels floats, uploaded per call into a grow-only buffer of the library's (the call waits for that copy, not for the
 * kernel).  out may be labels itself: each voxel reads and writes its own word, and the caller then reads the container as floats.  One
 * streaming pass; container padding is neither read nor written.  Refused (status 1, a message, nothing written): a null labels,
 * values or out; n_labels outside 1 .. 2^22; an empty box, one above 32768 along an axis or 2^31 - 1 voxels, or one that does not fit
 * the current container.  Geometry from the current container, library stream. */
int f3d_paint_labels(f3d_devptr labels, size_t n_labels, const float* values /* n_labels entries, host */, f3d_devptr out, size_t width,
                     size_t height, size_t depth);

/* Validation of a displacement (no reference counterpart: the normalised median test of PIV and volume-correlation post-processing,
 * Westerweel & Scarano 2005, which a workflow applies between the displacement and the strain).  A vector is compared with the median
 * of its neighbours, scaled by the median residual of those neighbours; a rejected vector becomes NaN (which f3d_flow_strain and
 * f3d_principal_strain treat as a missing sample) or the neighbour median.  Nothing is smoothed: a voxel is kept bit for bit, set to
 * NaN, or replaced by a median of input values.  Every operation is float32 and rounded on its own.
 *
 * Presence is f3d_motion_sums': a voxel is present when it is inside the volume, none of u, v, w is NaN there and, when weight is
 * not 0, weight[i] >= weight_min (a NaN weight fails the comparison).
 * Neighbours of voxel p are the up to 26 points p + step * (i, j, k), (i, j, k) in {-1, 0, 1}^3 without (0, 0, 0), that lie inside
 * the volume and are present; there is no mirroring.  k is their number.  (The dense flow is smooth at the scale of a voxel and its
 * errors are blobs, so the neighbours are taken step voxels away; step = 1 is the classic test.)
 * The median of k >= 1 values s_0 <= ... <= s_{k-1} is s_{(k-1)/2} for odd k and 0.5f * (s_{k/2-1} + s_{k/2}) for even k.
 * Per component c of d = (u, v, w):
 *   med_c = the median of the neighbours' d_c;  rm_c = the median of fabsf(n_c - med_c) over the same neighbours;
 *   r_c = fabsf(d_c - med_c) / (rm_c + eps), IEEE division;   r = fmaxf(fmaxf(r_u, r_v), r_w).
 * Classes: tested = present and k >= min_neighbours; outlier = tested and r > threshold; kept = present and not an outlier (a present
 * voxel with too few neighbours is kept, untested); every other voxel is rejected: the outliers and the absent voxels, those absent
 * only by the weight included (this is how a zncc mask is applied).  threshold = +inf is accepted: nothing is an outlier, and the call
 * only fills absent voxels.
 *   out[0]     (F3D_VALIDATE_R)  r where tested, NaN elsewhere
 *   out[1..3]  (F3D_VALIDATE_D)  a kept voxel bit for bit; a rejected voxel NaN in all three under F3D_VALIDATE_MARK; under
 *              F3D_VALIDATE_REPLACE (med_u + 0.f, med_v + 0.f, med_w + 0.f) when k >= min_neighbours and NaN in all three otherwise.
 *              The + 0.f stores a zero median as +0: which of several zeros of mixed sign is the middle one is not defined, and
 *              nothing else depends on that sign.  One Jacobi pass: the medians are of the input, an outlier neighbour still votes.
 * stats (nullable; asking waits for the stream): present, tested, outliers count the classes; replaced counts rejected voxels that
 * received a median (0 under MARK); undefined counts voxels whose validated u is NaN (whether or not D is stored); r_max is the exact
 * maximum of r over the tested voxels, NaN when there are none.  They are combined in the fixed order of the other statistics (the
 * xor butterfly over the 64 x of a wave, the 4 rows of a workgroup, the fold of the workgroup partials), no float atomics: the same
 * input gives the same bytes.  Infinite inputs are outside the definition.
 * Geometry from the current container (f3d_set_container), whole volume, library stream.  Refused (status 1, a message, nothing
 * written): a null u, v or w; a null selected output; fields 0 or with unknown bits; an unknown mode; step outside 1 .. 16;
 * min_neighbours outside 1 .. 26; eps NaN, infinite or not above 0; threshold NaN or negative; a NaN weight_min when a weight is
 * given; a selected output that is also an input (the weight included) or the container of another selected output; an empty size. */
#define F3D_VALIDATE_R 1u       /* out[0]      r, the normalised residual            */
#define F3D_VALIDATE_D 2u       /* out[1..3]   the validated u, v, w                 */
#define F3D_VALIDATE_MARK 1u    /* rejected voxels become NaN                        */
#define F3D_VALIDATE_REPLACE 2u /* rejected voxels become the neighbour median       */
typedef struct f3d_validate_stats {
  unsigned long long present, tested, outliers, replaced, undefined;
  float r_max;
} f3d_validate_stats;
int f3d_validate_displacement(f3d_devptr u, f3d_devptr v, f3d_devptr w, f3d_devptr weight /* 0: none */, float weight_min,
                              unsigned step, float eps, float threshold, unsigned min_neighbours, unsigned mode,
                              const f3d_devptr out[4], unsigned fields, size_t width, size_t height, size_t depth,
                              f3d_validate_stats* stats /* nullable; non-null waits */);

#ifdef __cplusplus
}
#endif
#endif /* F3D_H_ */
