/* gpismap_amd -- C-ABI of the MI355X-native GPisMap hot path.
 *
 * Plain pointers and sizes only; every function returns an int status
 * (0 = GPIS_OK, negative = error) unless stated otherwise and never throws.
 * Host pointers unless a parameter is named d_* (device pointer).
 *
 * Map level: what a binding of the reference's mex gateways would call.
 *   reference mex/mexGPisMap3.cpp:  'update' :49-78, 'test' :79-110,
 *   'setCamera' :111-144, 'getAllPoints' :145-157, 'reset' :158-166
 *   -> class GPisMap3  reference cpp/include/GPisMap3.h:117-127
 *   reference mex/mexGPisMap.cpp:   'update' :40-85, 'test' :86-122, 'reset' :123-131
 *   -> class GPisMap   reference cpp/include/GPisMap.h:97-106
 * Kernel level: the batched GP primitives.
 */
#ifndef GPISMAP_AMD_H_
#define GPISMAP_AMD_H_

#ifdef __cplusplus
extern "C" {
#endif

#define GPIS_OK 0
#define GPIS_ERR_ARG (-1)
#define GPIS_ERR_HIP (-2)
#define GPIS_ERR_STATE (-3)
#define GPIS_ERR_LIMIT (-4)

typedef struct gpis_cam {  /* reference camParam, GPisMap3.h:29-46 */
    float fx, fy, cx, cy;
    int width, height;
} gpis_cam;

/* number of HIP devices visible (0 when no GPU: every compute entry then fails loudly) */
int gpis_device_count(void);
/* The library keeps the standard-size chunks of destroyed device pools per device for the next map of the process (bounded by
 * GPIS_POOL_CACHE_GB, default 16).  gpis_pool_cache_trim() hands them back to the driver -- call it when another library in the
 * process needs the memory; returns the bytes released.  No map may be in use on another thread during the call. */
unsigned long long gpis_pool_cache_trim(void);
const char* gpis_version(void);
/* Device selection (one process per GPU in a multi-GPU job: call once with LOCAL_RANK before creating anything).
 * Every object created afterwards lives on the device current at its creation and makes it current inside each
 * call; d_* pointers and streams handed to *_test_device must belong to that device.  GPIS_ERR_ARG if out of range. */
int gpis_set_device(int device);
int gpis_get_device(void);

/* ---- 3-D map (GPisMap3) -------------------------------------------------- */
void* gpis3_create(const gpis_cam* cam /* NULL = reference defaults */);
/* ONE map object over several devices of this process (a device may be listed more than once: logical shards on one GPU).
 * update() runs on every listed device from its own host thread, each trains its K^3-balanced share of the frame's
 * clusters, the packed models are copied device to device and every device ends up with the whole map; test() deals the
 * queries to the devices in blocks of 65 536 and answers them concurrently.  Results are bit-identical to a one-device
 * map.  The GPisMap3 class does the same when GPIS_DEVICES=0,1,... is set in the environment (so the unchanged mex
 * gateway uses every GPU).  Reference: the fan-out over host threads, GPisMap3.cpp:759-784 (updateGPs), :904-949 (test). */
void* gpis3_create_multi(const gpis_cam* cam /* NULL = reference defaults */, const int* devices, int n);
int   gpis3_num_devices(void* map);
void  gpis3_destroy(void* map);
int   gpis3_reset(void* map);                                   /* GPisMap3::reset    GPisMap3.cpp:99  */
int   gpis3_set_camera(void* map, const gpis_cam* cam);         /* GPisMap3::resetCam GPisMap3.cpp:117 */
/* depth: width*height floats, column-major (index = col*height + row), metres;
 * pose12 = [t(3), R column-major(9)].                          GPisMap3::update GPisMap3.cpp:218 */
int   gpis3_update(void* map, const float* depth, int n, const float* pose12);
/* x: n*3 interleaved; res: n*8 [f gx gy gz vf vgx vgy vgz], pre-filled by the caller; only the
 * entries the reference writes are touched.  Returns GPIS_ERR_ARG where the reference returns
 * false; a failure of the device path is never folded into that: GPIS_ERR_HIP / _STATE / _LIMIT.
 *                                                             GPisMap3::test GPisMap3.cpp:904 */
int   gpis3_test(void* map, const float* x, int dim, int n, float* res);
int   gpis3_test_device(void* map, const float* d_x, int n, float* d_res, void* hip_stream);
int   gpis3_device(void* map);                                 /* device the map lives on, or negative */
/* ---- multi-GPU: sharded cluster training (one process per GPU).  Every rank runs the same update()
 * (host logic is deterministic, so trees, cluster sets and model slots agree), but after gpis3_set_shard(rank, world)
 * it TRAINS only its share of the frame's clusters (greedy longest-processing-time partition by K^3).  The caller then
 * moves the packed models between the ranks and completes the update.  A rank's records (what prediction reads of each of
 * its models: 2 K^2 + 20 K bytes) sit BACK TO BACK at their own sizes in the frame's job order; every rank can size every
 * rank's buffer (gpis3_shard_bytes), so an exchange moves the records' bytes and no padding between them:
 *   gpis3_update(...);                                  trains the local share, defers the cluster table
 *   gpis3_shard_info(map, out, 2 + world)               out[0] = clusters of this frame, out[1] = local ones,
 *                                                       out[2 + r] = clusters rank r trains
 *   gpis3_shard_bytes(map, r)                           bytes of rank r's records (the same answer on every rank)
 *   gpis3_shard_pack(map, d_send, stream)               local models -> d_send[0 .. gpis3_shard_bytes(map, rank))
 *   ... transport: e.g. one RCCL all_gather_into_tensor of buffers padded to the largest RANK total (the K^3-balanced
 *       partition makes the totals near-equal), grouped send/recv, or hipMemcpyPeerAsync inside one process ...
 *   gpis3_shard_unpack(map, r, d_recv_r, stream)        for every other rank r
 *   gpis3_shard_finish(map)                             builds the cluster table: test() is valid again
 * With world = 1 (default) update() is complete on return and none of the calls is needed. */
int   gpis3_set_shard(void* map, int rank, int world);
/* What the records of a sharded update carry (same size either way): mode 1 = FACTOR records for models whose explicit inverse is
 * still pending (lazy inverse: -L re-tiled + alpha; the receiver computes X = L^-1 when it first predicts with the model, so no
 * rank inverts a cluster that is retrained before anybody asks), mode 0 = prediction records (X; packing forces the inverse on
 * the owner), mode -1 (default) = 1 with the lazy inverse, 0 with the eager one.  Also applies to maps over several devices.
 * gpis3_stats out[27] = factor records received in the last exchange. */
int   gpis3_set_shard_factors(void* map, int mode);
int   gpis3_shard_info(void* map, int* out, int n);
long long gpis3_shard_bytes(void* map, int owner);
int   gpis3_shard_pack(void* map, void* d_buf, void* hip_stream);
int   gpis3_shard_unpack(void* map, int owner, const void* d_buf, void* hip_stream);
int   gpis3_shard_finish(void* map);
/* One process per GPU, the host logic of update() run ONCE (round 6).  By default every rank of a sharded run replays the whole
 * frame (tree mutation, ObsGP round trips: the larger half of an update) and only the training is divided.  Alternatively the
 * LEAD rank (rank 0 of gpis3_set_shard) records what its update() decided and the other ranks apply the record:
 *   lead:    gpis3_set_frame_export(map, 1) once;  per frame  gpis3_update(...)           host logic, record written, own share NOT trained yet
 *                                                             n = gpis3_frame_record(map, buf, cap)   (a few hundred KB .. MB: the point mirror dominates)
 *                                                             ... broadcast buf[0..n) to the workers ...
 *                                                             gpis3_train_deferred(map)   the lead's own share
 *   worker:  per frame  gpis3_apply_frame(map, buf, n)        slot operations mirrored (the ids must come out as the lead's), point
 *                                                             mirror uploaded, K6 on its own device, its share trained
 *   all:     the exchange as above (gpis3_shard_info / _bytes / _pack / _unpack / _finish).
 * gpis3_frame_record returns the record's size (copies it when cap suffices); a worker map never calls gpis3_update (it holds no
 * tree: gpis3_get_points answers on the lead only) and is created for that role: gpis3_apply_frame on a map that has replayed
 * frames itself returns GPIS_ERR_STATE.  gpis3_stats out[26] (host replays of the last update) is 1 on the lead and 0 on a worker.
 * reset / loadMap on the lead are not recorded: recreate the workers with it. */
int   gpis3_set_frame_export(void* map, int on);
long long gpis3_frame_record(void* map, void* buf, long long cap);
int   gpis3_train_deferred(void* map);
int   gpis3_apply_frame(void* map, const void* buf, long long bytes);
int   gpis3_num_points(void* map);
int   gpis3_get_points(void* map, float* out3, int cap);        /* GPisMap3::getAllPoints GPisMap3.cpp:951 */
int   gpis3_get_nodes(void* map, float* out9, int cap);         /* pos3 grad3 val sigx sigg, tree order */
/* out[0..27]: obsgp groups trained, obsgp queries, clusters trained (cumulative), late re-evaluations, clusters in table,
 * GP evaluations of last test, ms in K4 of last test (profiling on), device bytes, algorithmic flops of last test, K4 launches,
 * ms in K6+K3+K3b of last update (profiling on), model bytes, update phases ms [preproc, ObsGP train, re-evaluation,
 * new points, updateGPs], algorithmic flops / bytes / clusters / largest K of the last training batch, ms and clusters of the
 * last deferred inverse pass (profiling on), bytes received in the last in-library model exchange, pipelined update on (0/1),
 * CUs the training streams leave free, host replays of the last update() over all devices of the map (1: the host logic ran
 * once, on the lead device, however many devices train), factor records received in the last model exchange (inverses deferred) */
int   gpis3_stats(void* map, double* out, int n);
/* K4 evaluations of the last test() by kind: [0] pass 1 (nearest candidate, all columns), [1] candidate 2 of two-candidate
 * queries (all columns), [2] value columns of candidates 2 and 3 of three-candidate queries, [3] the records among those that
 * the blend reads in full (their gradient columns are needed) -- the same numbers in every pass-2 mode, whichever pass and
 * layout did the work.  The flops of gpis3_stats count the columns computed: in the predicting modes they include the
 * gradient columns of a candidate that was evaluated in full and then not read. */
int   gpis3_pass_jobs(void* map, long long* out4);
/* How test() evaluates candidates 2 and 3 of a three-candidate query whose first variance is above the threshold.  The blend
 * reads in full almost always exactly one of them.  0: the value column of both, then the gradient columns of the records the
 * blend reads.  1 (default): a predictor picks one from the query's distances to the models' points; that one is evaluated in
 * full together with the two-candidate jobs, the other gets its value column, and gradient columns are computed afterwards
 * only where the prediction missed or both are read.  2 / 3: always candidate 2 / 3 in full.  4: the predictor inverted (for
 * tests of the repair path).  The results are the same bits in every mode; only the time differs.  The environment variable
 * GPIS_PASS2 sets the initial mode of a new map.  Takes effect at the next test().  GPIS_ERR_ARG outside 0..4. */
int   gpis3_set_pass2_mode(void* map, int mode);
/* How test() cuts a call into chunks, each of which runs every pass (one prediction launch per cluster size class and pass).
 * 0: chunks of 2^22 queries.  1 (default): the whole call in one chunk where the device has the memory, as
 * gpis_mapquery_set_chunk(mq, 0) describes: the per-chunk work and the drained device at the end of every launch are paid once.
 * The results are the same bits in both; only the time differs.  The environment variable GPIS_K4_SCHEDULE sets the initial mode
 * of a new map.  Takes effect at the next test().  GPIS_ERR_ARG outside 0..1. */
int   gpis3_set_k4_schedule(void* map, int mode);
/* out[0..7] of the last test(): evaluations in full of a predicted candidate, value-column-only evaluations, gradient-column
 * evaluations afterwards, predicted candidates evaluated in full that the blend did not read, predictions made (both candidates
 * have a model), predictions the blend read, ms in the predictor kernel (profiling on), the mode.  out[0] + out[1] = [2] and
 * out[2] + out[0] - out[3] = [3] of gpis3_pass_jobs. */
int   gpis3_pass_detail(void* map, double* out8);
/* Map checkpoint (optional; the reference keeps its map only in the mex singleton): gpis3_save writes the spatial
 * index, the surface points with their data and every trained model as its packed prediction record (about 2 K^2 bytes per
 * cluster: the file of a 500-cluster map is ~1.2 GB) (GPisMap3::saveMap); gpis3_load replaces the map's state with a file's.
 * Nothing is retrained -- the records are restored verbatim, so test() answers with the same bits as before the save and the
 * next update continues from it; restored models are predict-only until their cluster is trained again.  The file is a raw image
 * of this build's structures with a checksum over the payload: another build's, a truncated or a damaged file is refused
 * (GPIS_ERR_ARG) and the map stays as it was.  The camera is not part of it. */
int   gpis3_save(void* map, const char* path);
int   gpis3_load(void* map, const char* path);
int   gpis3_set_profile(void* map, int on);
/* Pipelined update (the default since round 4; gpis3_set_pipeline(map, 0) or GPIS_PIPELINE_UPDATE=0 in the environment select
 * the reference's synchronous update(), GPisMap3.cpp:218-237): gpis3_update() returns once the frame's OnGPIS training is
 * enqueued; the next update's training, test, the getters, statistics and the sharded exchange join it first, so results never
 * depend on the mode -- only WHEN a training failure is reported does: by the call that joined.  gpis3_sync() joins explicitly
 * and returns the pending update status.  While it is on, the training streams are kept off GPIS_PIPELINE_RESERVE_CUS CUs
 * (default 32, spread evenly over the XCDs) so that the next frame's ObsGP batches never wait for a factorisation workgroup.
 * Maps that shard their training over ranks or devices run synchronously whatever the setting (every frame ends with the
 * exchange). */
int   gpis3_sync(void* map);
int   gpis3_set_pipeline(void* map, int on);
/* Cross-check paths, reachable through these setters only (no environment switch since round 5):
 *  - K6's range part (which points of the touched cells lie in a cluster's range, GPisMap3.cpp:721-735) runs on the device;
 *    gpis3_set_host_gather(map, 1) selects the host walk it replaced -- same training sets;
 *  - a cluster keeps only what prediction reads once its inverse exists; gpis3_set_keep_factors(map, 1) keeps the training side
 *    (factor, re-tiled factor) of every model as well (10 K^2 instead of 2 K^2 bytes per cluster). */
int   gpis3_set_host_gather(void* map, int on);
int   gpis3_set_keep_factors(void* map, int on);
/* Lazy inverse at map level (default on; GPIS_EAGER_INVERSE=1 or gpis3_set_lazy_inverse(map, 0) turn it off): update() trains
 * factors and alpha; the explicit inverses are computed by the first test() after it (or by gpis3_prepare_test(), which also
 * joins a pipelined training) -- once per cluster, however many updates retrained it in between.  With a test() after
 * every update() the total work is unchanged; with several updates per test() the inverses of the intermediate factors
 * are never computed.  Results do not depend on the mode. */
int   gpis3_prepare_test(void* map);
int   gpis3_set_lazy_inverse(void* map, int on);

/* ---- 2-D map (GPisMap) ---------------------------------------------------- */
void* gpis2_create(void);                                       /* GPisMap() GPisMap.cpp:57 */
void  gpis2_destroy(void* map);
int   gpis2_reset(void* map);                                   /* GPisMap::reset GPisMap.cpp:90 */
/* thetas / ranges: n floats each (radians, metres); pose6 = [tx ty R11 R21 R12 R22].
 *                                                               GPisMap::update GPisMap.cpp:151 */
int   gpis2_update(void* map, const float* thetas, const float* ranges, int n, const float* pose6);
/* x: n*2 interleaved; res: n*6 [f gx gy vf vgx vgy], pre-filled by the caller.  GPisMap::test GPisMap.cpp:765 */
int   gpis2_test(void* map, const float* x, int dim, int n, float* res);
int   gpis2_test_device(void* map, const float* d_x, int n, float* d_res, void* hip_stream);
int   gpis2_device(void* map);
/* Round 6: the 2-D update() is pipelined like the 3-D one -- it returns once the frame's OnGPIS training is enqueued; the next
 * update, gpis2_test / _test_device, gpis2_stats and gpis2_sync join it (a failed training surfaces there).  gpis2_set_pipeline(map, 0)
 * or GPIS_PIPELINE_UPDATE=0 restore the synchronous call.  Same map state and test() results in both modes. */
int   gpis2_sync(void* map);
int   gpis2_set_pipeline(void* map, int on);
int   gpis2_get_nodes(void* map, float* out7, int cap);         /* pos2 grad2 val sigx sigg, tree order */
int   gpis2_stats(void* map, double* out, int n);               /* same slots as gpis3_stats */
int   gpis2_pass_jobs(void* map, long long* out4);              /* same slots as gpis3_pass_jobs */
int   gpis2_set_pass2_mode(void* map, int mode);                /* as gpis3_set_pass2_mode */
int   gpis2_pass_detail(void* map, double* out8);               /* same slots as gpis3_pass_detail */

/* ---- kernel level: observation GP (K1, K2) -------------------------------- */
void* gpis_obsgp_create(void);
void  gpis_obsgp_destroy(void* g);
/* ObsGP2D::train ObsGP.cpp:331: vu = ni*nj interleaved (v,u), f = ni*nj (valid iff > 0) */
int   gpis_obsgp_train2d(void* g, const float* vu, const float* f, int ni, int nj);
/* ObsGP1D::train ObsGP.cpp:85 */
int   gpis_obsgp_train1d(void* g, const float* theta, const float* f, int n);
/* batched single-point queries (ObsGP2D::test ObsGP.cpp:410 / ObsGP1D::test :145);
 * q: nq*2 (2-D) or nq (1-D); val is pre-filled by the caller and left untouched where no
 * group answers (var = 1e6 there) */
int   gpis_obsgp_query(void* g, const float* q, int nq, float* val, float* var);
/* The same batch through one of the routes update() takes (kernel-level tests of the staging paths): route 0 = gpis_obsgp_query;
 * 1 = page-locked staging, the kernel working on it directly below 4096 queries; 2 = the second staging set, asynchronous on
 * a stream of its own, then waited for.  Routes 1 and 2 start from val = 0 (a miss leaves 0 and var = 1e6).  Route 3 is the
 * first half of route 2 (returns with the batch pending; val / var untouched), route 4 the second (waits, copies the
 * answers of that batch; q is not read; GPIS_ERR_STATE when route 3 left none, GPIS_ERR_ARG when nq is not its size).  A
 * training call issued in between waits for the batch: gpis_obsgp_pending() is 1 from route 3 until then, else 0. */
int   gpis_obsgp_query_route(void* g, int route, const float* q, int nq, float* val, float* var);
int   gpis_obsgp_pending(void* g);
int   gpis_obsgp_num_groups(void* g);
int   gpis_obsgp_get_group(void* g, int group, int* n, float* x128, float* alpha64, float* L4096);

/* ---- kernel level: OnGPIS batches (K6, K3, K4) ----------------------------- */
void* gpis_ongpis_create(int dim, float scale);
void  gpis_ongpis_destroy(void* s);
/* points: 9 SoA rows of length npts (px py pz gx gy gz val sigx sigg); clusters given as CSR
 * (off[ncl+1], ids[]) of point ids in training order.  model_out[ncl] receives the model slots.
 * OnGPIS::train OnGPIS.cpp:91-149 (2-D :34-89) for every cluster. */
int   gpis_ongpis_train(void* s, const float* points_soa9, int npts, const int* off, const int* ids, int ncl,
                        int* model_out);
/* copy a trained model back: sizes via gpis_ongpis_model_dims (N, ng, K, ld) */
int   gpis_ongpis_model_dims(void* s, int model, int* dims4);
int   gpis_ongpis_get_model(void* s, int model, float* L_ldxld, float* alpha_K, int* gidx_N);
/* OnGPIS::testSinglePoint OnGPIS.cpp:177-216 (2-D test2Dpoint :218) for njobs (query, model) pairs.
 * xq: nq*dim interleaved; out: njobs*8 = mean(4) var(4) (2-D uses 3+3, slots 3 and 7 unused) */
int   gpis_ongpis_eval(void* s, const float* xq, int nq, const int* job_q, const int* job_model, int njobs,
                       float* out8);
/* the same for a subset of the result columns: layout 0 = all (= gpis_ongpis_eval), 1 = component 0 (mean f, value variance),
 * 2 = components 1..dim (gradient and its variances); the slots of the other components are 0 */
int   gpis_ongpis_eval_layout(void* s, const float* xq, int nq, const int* job_q, const int* job_model, int njobs, int layout,
                              float* out8);
/* Rounds 2-4: K4 kept one double-precision exp per (training point, query) in an LDS table when it fit.  The kernel since round 5
 * (B chunks in a three-slot ring) spends that LDS on wider chunks and evaluates the exponential per entry for every cluster:
 * gpis_ongpis_set_exp_table is accepted for compatibility and changes nothing (results were identical either way). */
/* Packed model records for a multi-GPU exchange (what K4 needs from a trained model: 2 K^2 + 20 K bytes): pack the listed
 * models into d_buf (n records of `stride` bytes, stride >= gpis_ongpis_packed_bytes of every sender, a multiple of 256),
 * unpack records into predict-only models (models_inout[i] < 0: a new model is created and its id returned). */
long long gpis_ongpis_packed_bytes(void* s, const int* models, int n);
int   gpis_ongpis_pack(void* s, const int* models, int n, void* d_buf, long long stride, void* hip_stream);
int   gpis_ongpis_unpack(void* s, const void* d_buf, int n, long long stride, int* models_inout, void* hip_stream);
int   gpis_ongpis_set_exp_table(void* s, int on);
/* Clusters of at most 256 rows are trained by one fused on-chip kernel and keep only what prediction reads
 * (row table, points, the re-tiled inverse factor).  keep_factor(1) BEFORE training makes such models carry L, alpha
 * and gidx as well (gpis_ongpis_get_model returns GPIS_ERR_STATE for a model without them); set_fused(0) sends every
 * cluster through the separate gather / build / factorise / invert kernels (same results, bit for bit). */
/* kernel matrix only (the build kernel on caller-given arrays, no gather rule): x [n][dim], gidx [n] running gradient
 * index or -1, sigx / sigg [n]; K_out receives the K x K lower triangle, column-major, K = n + dim * #(gidx >= 0).
 * reference matern32_sparse_deriv1_3D / _2D (train), covFnc.cpp:142-256 / :317-402 */
int   gpis_ongpis_kernel_matrix(void* s, const float* x, const int* gidx, const float* sigx, const float* sigg, int n, float* K_out);
int   gpis_ongpis_set_keep_factor(void* s, int on);
int   gpis_ongpis_set_fused(void* s, int on);
/* Lazy inverse (default on): training of clusters of more than 256 rows stops at the factor and alpha (what
 * OnGPIS::train computes, OnGPIS.cpp:139-143); the explicit inverse the prediction kernel multiplies with is computed at the
 * first prediction / packing after a training, once per cluster however often it was retrained in between.  on = 0: the
 * inverse runs behind the factorisation in every training batch. */
int   gpis_ongpis_set_lazy_inverse(void* s, int on);
/* In-kernel waits (the cooperative factorisation of the largest clusters, the pipelined inverse) are bounded: when one
 * expires the batch's models are dropped and training returns GPIS_ERR_STATE.  wait_limit_ms = 0 keeps the default
 * (2 s); inject is a TEST hook: bit 0 makes one workgroup of every cooperative cluster withhold a hand-over; bit 4 (16)
 * makes the first workgroup of every prediction launch withhold one signal of its LDS ring (and shortens that kernel's
 * bounded wait): its tile's results are NaN, the error word of the launch is raised and gpis_ongpis_eval / test() return
 * GPIS_ERR_STATE -- so that the error paths can be exercised. */
int   gpis_ongpis_set_debug(void* s, int inject, int wait_limit_ms);
/* CUs the training streams of this handle leave free (what the maps do for their pipelined update: gpis3_set_pipeline /
 * GPIS_PIPELINE_RESERVE_CUS).  The streams are created with a CU mask over the first (CUs - n) bits -- bit i is CU i / 8 of XCD
 * i % 8 -- and the cooperative factorisation sizes its workgroup groups for what is left on one XCD.  0 = ordinary streams. */
int   gpis_ongpis_set_cu_reserve(void* s, int n);
/* Device self-test (round 6): the factorisation kernels take their square roots and divisions through range-restricted sequences
 * (csrc/tile_solve.h: the compiler's correctly rounded expansions without the operand scaling and classification the chains'
 * operands never need).  Runs blocks * 256 * per_thread random operand pairs through them and through the compiler's sqrtf and `/`
 * on the current device and returns the number of results whose bits differ: mismatches2[0] square roots, [1] divisions.
 * mode 0: the documented operand ranges; mode 1: operands shaped like the factorisations'; mode 2: the table-driven double-precision
 * exponential of the prediction / query kernels (csrc/exp_tab.h) against the device library's exp on arguments in [-12, 0] and a
 * few deep in the underflow range: mismatches2[0] = results more than one ulp apart, [1] = results that differ at all. */
int   gpis_selftest_ranged_arith(unsigned long long seed, int blocks, int per_thread, int mode, unsigned long long* mismatches2);
int   gpis_ongpis_last_ms(void* s, float* train_ms, float* eval_ms);

/* ---- kernel level: K5, the driver of test() (lookup, binning, passes, blend) on a caller-given cluster table -------------
 * A probe for tests: the MapQuery the maps use, over the store of a gpis_ongpis_create handle (its device, its stream, its
 * dimension) and a synthetic table.  The handle must outlive the probe.  search_half: half side of the query box; var_thre:
 * the blend's gate; prior_var: the variance written before anything else.  NULL on a null handle or non-finite arguments. */
void* gpis_mapquery_create(void* ongpis, float search_half, float var_thre, float prior_var);
void  gpis_mapquery_destroy(void* mq);
/* The cluster table, entries in tree traversal order: centre c, box lo / hi ([ncl][3], the third 0 in 2-D), model = a trained
 * slot of the store or -1, parent = index of the first ancestor or -1; ancestors: boxes and the next ancestor (an EARLIER index
 * or -1).  Centres lie on a lattice of `pitch`.  Checked on the host before anything reaches a kernel: null handle, ncl < 0,
 * a parent or model out of range, an ancestor parent that is not an earlier one -> GPIS_ERR_ARG; two centres in one lattice
 * cell -> GPIS_ERR_STATE.  May be called again on a live handle (any size). */
int   gpis_mapquery_set_table(void* mq, int ncl, const float* c, const float* lo, const float* hi, const int* model,
                              const int* parent, int nanc, const float* anc_lo, const float* anc_hi, const int* anc_parent,
                              double pitch);
/* queries per pass of the chunk loop (the results do not depend on it); negative -> GPIS_ERR_ARG.  0 (the default) = automatic:
 * the whole call in one chunk when its scratch (about 156 bytes per query) fits in one eighth of the free device memory, halved
 * until it does, never below 2^22 and never above 2^28; 2^22 under K4 schedule 0. */
int   gpis_mapquery_set_chunk(void* mq, int n);
/* x [n][dim], res [n][2(1+dim)] host arrays; res is uploaded first (as gpis3_test does): only the entries the reference
 * writes change.  n = 0 is a no-op. */
int   gpis_mapquery_run(void* mq, const float* x, int n, float* res_inout);
/* The same run on the caller's device buffers (on the probe's device), as gpis3_test_device: d_x [n][dim], d_res_inout
 * [n][2(1+dim)], on hip_stream (NULL: the store's stream).  Work queued on another stream that writes the buffers must have
 * finished.  Synchronous on return; the same refusals as gpis_mapquery_run. */
int   gpis_mapquery_run_device(void* mq, const float* d_x, int n, float* d_res_inout, void* hip_stream);
/* the lookup's result of the last run: ncand [n], cand [3][n] (model slot or -1).  Only after a run of one chunk over a
 * non-empty table, GPIS_ERR_STATE otherwise. */
int   gpis_mapquery_candidates(void* mq, int* ncand, int* cand3);
/* K4 jobs of the last run per pass: 1, 2 (two-candidate queries, all columns), 2a (value column), 2b (gradient columns) */
int   gpis_mapquery_pass_jobs(void* mq, long long* out4);
/* as gpis3_set_pass2_mode / gpis3_pass_detail / gpis3_set_k4_schedule */
int   gpis_mapquery_set_k4_schedule(void* mq, int mode);
/* of the last run: evaluations, K4 launches, queries per chunk, the K4 schedule in force */
int   gpis_mapquery_last_counts(void* mq, long long* out4);
int   gpis_mapquery_set_pass2_mode(void* mq, int mode);
int   gpis_mapquery_pass_detail(void* mq, double* out8);

/* ---- surface extraction: the map's zero-level surface on the device (DESIGN.md "Surface extraction") ------------------
 * The map's test() on a lattice of nx x ny (x nz) points (index p = (k ny + j) nx + i, x fastest; coordinates
 * origin + (float)i * step per axis, float32, no FMA), f = slot 0 of each zero-prefilled record; marching tetrahedra on the
 * Freudenthal split of every cell (6 tetrahedra per cube, 2 triangles per square) at `level` (inside iff f < level; NaN =
 * -fbias of the map's parameters, the level its surface points are stored at); then the map's test() on the vertices.
 * One vertex per crossed lattice edge, numbered in edge order; triangles (3-D) are wound so that cross(v1 - v0, v2 - v0)
 * points to f >= level and start at their smallest index, segments (2-D) have the right-hand normal (dy, -dx) pointing
 * there; primitives come by cell, then simplex.  Every position comes from an exclusive scan: the same bits on every run.
 * A mesh object is a result holder whose device buffers (about 13 B per lattice point plus the output) are reused across
 * calls; every extraction returns with its work finished.  Arguments: a size < 2 on any axis, a non-finite origin, a
 * non-positive or non-finite step, null pointers -> GPIS_ERR_ARG, the previous result untouched.  More than 2^28 lattice
 * points -> GPIS_ERR_LIMIT before anything is allocated; 2^31 or more vertices or primitives -> GPIS_ERR_LIMIT before the
 * output is allocated.  Any other failure (the test() path's status propagates: GPIS_ERR_STATE on an expired K4 ring wait,
 * ...) leaves no result (counts 0).  An empty surface is a result: 0 vertices, 0 primitives. */
void* gpis_mesh_create(void);                              /* on the current device; NULL without one */
void  gpis_mesh_destroy(void* mesh);
/* lattice points per test() pass of a map-level extraction (test hook: the results do not depend on it); 0 = 2^22 */
int   gpis_mesh_set_chunk(void* mesh, int points);
/* kernel level: any device-resident value grid d_val[prod(n)] (x fastest) of the mesh's device, no map involved; dim 2 or 3,
 * level finite.  No vertex records (gpis_mesh_get's vrec must be NULL afterwards).  hip_stream NULL: the mesh's own stream. */
int   gpis_mesh_from_grid(void* mesh, const float* d_val, int dim, const int* n, const float* origin, const float* step,
                          float level, void* hip_stream);
/* map level: vertices [V][3], triangles [F][3], vertex records [V][8] (the map's test() record of every vertex: f, the
 * gradient -- the surface normal -- and the variances).  Behaves like gpis3_test_device: GPIS_ERR_STATE while a sharded update
 * is unfinished or when the map holds no tree, joins a pipelined training; a map over several devices extracts on its lead
 * device (same result as a one-device map).  hip_stream NULL: the map's stream. */
int   gpis3_extract_mesh(void* map, void* mesh, const int* n3, const float* origin3, const float* step3, float level,
                         void* hip_stream);
/* 2-D map: vertices [V][2], segments [S][2], vertex records [V][6] */
int   gpis2_extract_contour(void* map, void* mesh, const int* n2, const float* origin2, const float* step2, float level,
                            void* hip_stream);
int   gpis_mesh_counts(void* mesh, long long* nvert, long long* nprim);
/* host copies of the last result (any pointer may be NULL); vrec non-NULL after gpis_mesh_from_grid -> GPIS_ERR_STATE */
int   gpis_mesh_get(void* mesh, float* verts, int* prims, float* vrec);
/* the value grid (f, prod(n) floats) of the last map-level extraction; GPIS_ERR_STATE after gpis_mesh_from_grid */
int   gpis_mesh_get_grid(void* mesh, float* vals);
/* device pointers of the last result, valid until the next extraction or gpis_mesh_destroy (*d_vrec = NULL without records) */
int   gpis_mesh_device(void* mesh, const float** d_verts, const int** d_prims, const float** d_vrec);

/* ---- distance field: the map's signed Euclidean distance field on the device ------------------------------
 * The map's test() on the mesh's lattice (index p = (k ny + j) nx + i, x fastest; coordinates origin + (float)i * step,
 * float32, no FMA; f = slot 0 of each zero-prefilled record) with one step on every axis (cubic cells).  Inside iff f < level
 * (NaN = -fbias of the map's parameters); f NaN is unknown and counts as outside, so the sign is only as good as f.  max_var:
 * a point whose var_f (record slot 4 in 3-D, 3 in 2-D) is above it gets f = NaN first (+inf: no gate).  A site is a point with
 * a finite f and an axis neighbour with a finite f on the other side of the level; its anchor is the crossing of its crossed
 * axis edges closest to it along the edge's axis (ties: -x, +x, -y, +y, -z, +z), bit for bit the mesh vertex of that edge.
 * Every point takes the site q* of the smallest integer squared lattice distance (ties: the smallest index) -- an exact
 * Euclidean distance transform -- and dist = +-sqrtf of the float32 squared distance to q*'s anchor, negative iff inside;
 * d_min <= |dist| <= d_min + 2 step, d_min the distance to the nearest anchor.  No site at all: dist +-inf, site -1.  No atomics:
 * the same bits on every run and for any chunk size.  A field object is a result holder whose device buffers (about 28 B per
 * lattice point) are reused across calls; every call returns with its work finished.  Arguments: a size < 2 on any axis, a
 * non-finite origin, a non-positive, non-finite or anisotropic step, an infinite level, a NaN max_var, null pointers ->
 * GPIS_ERR_ARG, the previous result untouched.  More than 2^28 lattice points or more than 16384 on an axis -> GPIS_ERR_LIMIT
 * before anything is allocated.  Any other failure leaves no result. */
void* gpis_dfield_create(void);                            /* on the current device; NULL without one */
void  gpis_dfield_destroy(void* df);
/* lattice points per test() pass of a map-level call (test hook: the results do not depend on it); 0 = 2^22 */
int   gpis_dfield_set_chunk(void* df, int points);
/* kernel level: any device-resident f grid d_val[prod(n)] (x fastest) of the field's device, no map involved; dim 2 or 3, level
 * finite, step[dim] all equal.  hip_stream NULL: the field's own stream. */
int   gpis_dfield_from_grid(void* df, const float* d_val, int dim, const int* n, const float* origin, const float* step,
                            float level, void* hip_stream);
/* map level.  Behaves like gpis3_extract_mesh: GPIS_ERR_STATE while a sharded update is unfinished or when the map holds no
 * tree, joins a pipelined training; a map over several devices computes on its lead device.  hip_stream NULL: the map's stream. */
int   gpis3_distance_field(void* map, void* df, const int* n3, const float* origin3, const float* step3, float level,
                           float max_var, void* hip_stream);
int   gpis2_distance_field(void* map, void* df, const int* n2, const float* origin2, const float* step2, float level,
                           float max_var, void* hip_stream);
/* the last result's lattice: dim (0: no result), n[3], origin[3] (unused axes 1 and 0), the step */
int   gpis_dfield_info(void* df, int* dim, int* n3, float* origin3, float* step);
/* host copies of the last result, prod(n) each (any pointer may be NULL); no result -> GPIS_ERR_STATE; f non-NULL after
 * gpis_dfield_from_grid -> GPIS_ERR_STATE */
int   gpis_dfield_get(void* df, float* dist, int* site, float* f);
/* device pointers of the last result, valid until the next call or gpis_dfield_destroy (NULL where there is none) */
int   gpis_dfield_device(void* df, const float** d_dist, const int** d_site, const float** d_f);
/* d_out[m][1 + dim] = (d, dd/dx, dd/dy[, dd/dz]) at the device points d_x[m][dim]: the trilinear (2-D: bilinear) interpolant of
 * dist with u = (x - origin) / step per axis, i0 = min(floor(u), n - 2); a point with !(0 <= u <= n - 1) on any axis gives NaN.
 * No result -> GPIS_ERR_STATE.  hip_stream NULL: the field's own stream. */
int   gpis_dfield_sample(void* df, const float* d_x, long long m, float* d_out, void* hip_stream);

/* ---- rendering: depth images and laser scans from the map on the device --------------------------------
 * The inverse of update(): what the sensor would see from a pose.  Every ray is marched through the map's test(); every march
 * step is one test() pass over the rays still active, and nothing but one count per pass leaves the device.
 * 3-D rays: pixel (col, row) is ray k = col * height + row (update()'s column-major depth layout); u = ((float)col - cx) / fx,
 * v = ((float)row - cy) / fy; the ray parameter is the depth z; the world point is R[i] (u z) + R[3+i] (v z) + R[6+i] z + t[i]
 * evaluated left to right in float32 without FMA (update()'s expression, pose12 = [t(3), R(9)]); an arc-length step s is the
 * z step s / sqrt(u^2 + v^2 + 1).  2-D rays: beam theta has c = cos((double)theta), s = sin((double)theta) (host double, as
 * update()); local point ((float)(r c) + off0, (float)(r s) + off1) with the map's sensor offset, world R local + t
 * (pose6 = [t(2), R(4)]); the parameter is the range r and steps are metres.
 * Clip: [tnear, tfar] intersected with the box of all cluster cells of the map, grown by test()'s search half-width (slab test,
 * IEEE division); an empty interval is a miss (status 1) without any test().  Samples are test() records pre-filled with
 * f = NaN and zeros elsewhere: NaN = no cluster within the search box.  g = f - level.  Step: f NaN -> far_step (no point of that
 * segment lies in a cluster cell); otherwise clamp(|g|, min_step, max_step).  f is NOT a distance bound: max_step is what limits
 * tunnelling.  Hit: consecutive samples going from outside (g >= 0 or NaN) to inside (g < 0), both with var_f <= max_var
 * (otherwise the march goes on).  Refinement: `refine` bisection rounds on [z_prev, z] (midpoint lo + (hi - lo) * 0.5; NaN counts
 * as outside), then the secant point of the final bracket clamped into it (the top when g(lo) is NaN); one last test() gives the
 * output record there.  Status per ray: 0 hit, 1 left the clipped interval, 2 max_steps samples taken.  Rays without a hit
 * have depth NaN and an all-NaN record.  The active rays are compacted after every pass by an exclusive scan that keeps their
 * order: the same call gives the same bits every time, for any chunk size and either update mode.
 * Errors: a bad camera (size < 1, fx or fy zero or non-finite), a non-finite pose or beam angle, tnear < 0, tnear >= tfar,
 * non-positive or non-finite steps, min_step > max_step, refine outside [0, 64], max_steps < 1, an infinite level or a NaN max_var
 * -> GPIS_ERR_ARG, the previous result untouched; more than 2^26 rays -> GPIS_ERR_LIMIT before anything is allocated, the
 * previous result untouched.  Any other failure (no tree or an unfinished sharded update: GPIS_ERR_STATE; the test() path's
 * status) leaves no result.  A render object holds grow-only device buffers (about 150 B per ray) reused across calls; every
 * render returns with its work finished.  A map over several devices renders on its lead device. */
typedef struct gpis_render_opts {
    float tnear, tfar;          /* ray interval: depth (3-D) / range (2-D) */
    float min_step, max_step;   /* clamp of |g| as the arc-length step */
    float far_step;             /* step after a sample with f NaN; NaN = 0.9 x the map's search half-width */
    float level;                /* NaN = -fbias (the level of the map's surface points) */
    float max_var;              /* +inf: no variance test */
    int refine;                 /* bisection rounds */
    int max_steps;              /* samples per ray */
} gpis_render_opts;
/* defaults.  3-D: tnear 0.4, tfar 4 (update()'s valid range), min_step 1e-3, max_step 0.01, max_steps 512;
 * 2-D: tnear 0.2, tfar 30 (update()'s valid range), min_step 0.01, max_step 0.1, max_steps 1024; both: far_step NaN,
 * level NaN, max_var +inf, refine 8 */
int   gpis_render_default_opts(int dim, gpis_render_opts* opts);
void* gpis_render_create(void);                            /* on the current device; NULL without one */
void  gpis_render_destroy(void* render);
/* rays per test() call within a pass (test hook: the results do not depend on it); 0 = 2^22 */
int   gpis_render_set_chunk(void* render, int rays);
/* depth [W*H], record [W*H][8], status [W*H].  cam NULL: the map's camera; opts NULL: the defaults; hip_stream NULL: the map's */
int   gpis3_render_depth(void* map, void* render, const gpis_cam* cam, const float* pose12, const gpis_render_opts* opts,
                         void* hip_stream);
/* range [n], record [n][6], status [n].  More than 2^26 beams -> GPIS_ERR_LIMIT before thetas is read */
int   gpis2_render_scan(void* map, void* render, const float* thetas, int n, const float* pose6, const gpis_render_opts* opts,
                        void* hip_stream);
/* host copies of the last result (any pointer may be NULL); GPIS_ERR_STATE without one.  rec is [rays][2 (1 + dim)] after a map
 * render and [rays][1 + dim] after a field render (gpis_render_info's out[16] says which is held) */
int   gpis_render_get(void* render, float* depth, float* rec, unsigned char* status);
/* device pointers of the last result (NULL without one), valid until the next render or gpis_render_destroy */
int   gpis_render_device(void* render, const float** d_depth, const float** d_rec, const unsigned char** d_status);
/* out[0..n): rays, dim, test() passes (march + refinement + output), march passes, samples (rays over all passes), K4
 * evaluations, ms inside K4 (only while the map's profiling is on), hits, clip box lo[3], hi[3] (NaN for an empty map),
 * 1 if a result is held, ms of host wall time inside the test() passes (each ends synchronised), the kind of result held
 * (0 a map render, 1 a field render: gpis3_render_depth_field / gpis2_render_scan_field), the largest number of samples a single
 * ray took (field renders; 0 after a map render).  After a field render passes = march passes = 1 (the one kernel), samples
 * counts every sample of every ray, K4 evaluations and both ms are 0 and the clip box is the lattice's. */
int   gpis_render_info(void* render, double* out, int n);

/* ---- tracking: depth-camera and laser poses against the map on the device -----------------------------
 * The inverse question of rendering: from which pose does the sensor see this frame?  Damped Gauss-Newton on SE(3) (3-D) /
 * SE(2) (2-D); every iteration is one test() pass over the frame's points, whose residual and Jacobian terms are reduced to the
 * normal equations on the device; only the sums (29 / 11 doubles) leave it, and the host solves the 6x6 / 3x3 system.
 * 3-D points: update()'s sampling with obs_skip = stride: pixels (col, row) = (n stride, m stride), n < W / stride,
 * m < H / stride, column-major (k = col * H + row ascending), used iff 0.4 < (double)z < 4; u = ((float)col - cx) / fx,
 * v = ((float)row - cy) / fy, local point (u z, v z, z), world R[i] x + R[3+i] y + R[6+i] z + t[i] left to right in float32
 * without FMA, R and t the current double pose cast to float (pose12 = [t(3), R(9)] column-major): the point update() would
 * insert with that pose.  2-D points: beams with 0.2 < (double)r < 30 in input order, local ((float)(r c) + off0,
 * (float)(r s) + off1) with c, s = cos, sin((double)theta) on the host and the map's sensor offset, world R local + t
 * (pose6 = [t(2), R(4)]).  Records: test() pre-filled with f = NaN, zeros elsewhere.  r = f - level (float32); a point is an
 * inlier iff f and the gradient are finite, var_f <= max_var and |r| <= max_residual; Huber weight w = 1 if |r| <= huber, else huber / |r|.
 * Jacobian (double, from the float values; rotation about the sensor centre): 3-D J = [g ; (p - t) x g], xi = (v, omega);
 * 2-D J = [gx, gy, (px - tx) gy - (py - ty) gx]; p the float world point queried, t the float translation, g the gradient.
 * Sums over the inliers in double: the upper triangle of H = sum w J J^T, b = sum w J r, sum w r^2, the inlier count, reduced
 * by a fixed halving tree (segments of 256 points, then the segment partials): the same bits for every chunk size, launch
 * shape, update mode and device count.  Step: (H + damping diag(H)) delta = -b by Cholesky; R <- Exp(omega) R, t <- t + v
 * (Rodrigues in double; 2-D a rotation by omega).  Status: 0 converged (|v| < eps_t and |omega| < eps_r after a step),
 * 1 max_iters steps taken, 2 fewer than min_inliers inliers (the last good pose is returned), 3 a non-positive Cholesky pivot
 * (the pose is not moved).  The reported H, b, cost, inliers and residual image belong to the returned pose: after the last
 * step one more pass runs there (passes = iterations + 1; + 2 when status 2 follows a step).  max_iters = 0 evaluates the
 * given pose only.  A map without points is no error: status 2.
 * Errors: a bad camera (size < 1, fx or fy zero or non-finite), a non-finite pose or beam angle, n < 1, stride < 1,
 * max_iters < 0, min_inliers < 0, a negative or NaN max_residual / max_var / damping / eps, an infinite damping, huber <= 0 or
 * non-finite, an infinite level -> GPIS_ERR_ARG, the previous result untouched; more than 2^26 pixels / beams ->
 * GPIS_ERR_LIMIT before anything is allocated, the previous result untouched.  Any other failure (an unfinished sharded
 * update: GPIS_ERR_STATE; the test() path's status) leaves no result.  A tracker holds grow-only device buffers (about 60 B per
 * point, 8 B per pixel) reused across calls; every call returns with its work finished.  A map over several devices tracks
 * on its lead device. */
typedef struct gpis_track_opts {
    double max_residual;        /* inlier: |r| <= max_residual */
    double huber;               /* Huber threshold */
    double max_var;             /* inlier: var_f <= max_var (+inf: no variance test) */
    double damping;             /* lambda of (H + lambda diag(H)) */
    double eps_t, eps_r;        /* convergence: |v| < eps_t (m) and |omega| < eps_r (rad) */
    float level;                /* NaN = -fbias (the level of the map's surface points) */
    int stride;                 /* 3-D pixel stride (update()'s obs_skip); ignored in 2-D */
    int max_iters;              /* Gauss-Newton steps at most (0: evaluate the given pose) */
    int min_inliers;            /* fewer inliers: status 2 */
} gpis_track_opts;
/* defaults.  3-D: stride 2, max_residual 0.05, huber 0.01, min_inliers 100; 2-D: max_residual 0.5, huber 0.1, min_inliers 20;
 * both: max_var +inf, damping 1e-4, eps_t 1e-5, eps_r 1e-5, max_iters 20, level NaN */
int   gpis_track_default_opts(int dim, gpis_track_opts* opts);
void* gpis_track_create(void);                             /* on the current device; NULL without one */
void  gpis_track_destroy(void* tracker);
/* points per test() call within a pass (test hook: the results do not depend on it); 0 = 2^22 */
int   gpis_track_set_chunk(void* tracker, int points);
/* depth [W*H] column-major as update(); cam NULL: the map's camera; opts NULL: the defaults; pose12_out (may be NULL): the
 * returned pose; hip_stream NULL: the map's */
int   gpis3_track_depth(void* map, void* tracker, const gpis_cam* cam, const float* depth, const float* pose12_init,
                        const gpis_track_opts* opts, float* pose12_out, void* hip_stream);
/* thetas, ranges [n] as update().  More than 2^26 beams -> GPIS_ERR_LIMIT before thetas is read */
int   gpis2_track_scan(void* map, void* tracker, const float* thetas, const float* ranges, int n, const float* pose6_init,
                       const gpis_track_opts* opts, float* pose6_out, void* hip_stream);
/* host copies of the last result (any pointer may be NULL): H [n x n] row-major and b [n] (n = 6 / 3) at the returned pose,
 * the residual per pixel / beam (r of the inliers, NaN elsewhere); GPIS_ERR_STATE without one */
int   gpis_track_get(void* tracker, double* H, double* b, float* resid);
/* out[0..n): status, iterations, passes, points used, inliers, initial cost, final cost, ms of host wall time in the passes,
 * ms inside K4 (only while the map's profiling is on), 1 if a result is held, dim, pixels / beams, K4 evaluations */
int   gpis_track_info(void* tracker, double* out, int n);

/* ---- tracking against a distance field -----------------------------------------------------------------
 * gpis3_track_depth / gpis2_track_scan with the map's test() replaced by the field's sampler: the same points, Gauss-Newton
 * loop, statuses, reduction tree, options and result, with r = d, the sampled distance (gpis_dfield_sample's interpolant and
 * gradient at the fp32 world point of the pass: the field's level is zero by construction).  A point is an inlier iff d and its
 * gradient are finite and |(double)r| <= max_residual; there is no variance test (max_var was applied when the field was built)
 * and level is not read.  A point outside the lattice samples NaN and is no inlier.  Every pass is one fused kernel from the
 * local points (world point, sample, terms, the segment tree), the top tree and the one copy of 29 / 11 doubles; nothing is
 * written per point except the residual image, sampled again at the returned pose.  Same bits for every launch, stream, map
 * update mode and device count that built the same field.
 * map: may be NULL; it is read only for what the caller leaves NULL: the camera (cam NULL) in 3-D, the sensor offset (off2
 * NULL) in 2-D.  The map's tree, training and shard state are not used: a field from gpis_dfield_from_grid tracks without a
 * map.  The tracker moves to the field's device; hip_stream NULL: the field's own stream.  In gpis_track_info, K4
 * evaluations and ms are 0.
 * Errors: cam / off2 NULL without a map, a NULL field, depth, thetas or ranges, and gpis3_track_depth's argument errors (level
 * and max_var excepted) -> GPIS_ERR_ARG; a field of another dim -> GPIS_ERR_ARG; a field without a result -> GPIS_ERR_STATE;
 * more than 2^26 pixels / beams -> GPIS_ERR_LIMIT: all with the previous result untouched.  Any other failure leaves no result. */
int   gpis3_track_depth_field(void* map, void* df, void* tracker, const gpis_cam* cam, const float* depth,
                              const float* pose12_init, const gpis_track_opts* opts, float* pose12_out, void* hip_stream);
/* off2: the sensor offset (x, y) in the laser frame, NULL = the map's.  More than 2^26 beams -> GPIS_ERR_LIMIT before thetas is
 * read */
int   gpis2_track_scan_field(void* map, void* df, void* tracker, const float* thetas, const float* ranges, int n,
                             const float* off2, const float* pose6_init, const gpis_track_opts* opts, float* pose6_out,
                             void* hip_stream);

/* ---- rendering from a distance field --------------------------------------------------------------------
 * gpis3_render_depth / gpis2_render_scan with the map's test() replaced by the field's sampler (sphere tracing): the same rays,
 * parameter, world point, slab clip, hit rule, refinement, statuses and output layout, with these differences.
 * Clip box: the lattice, [origin, origin + (float)(n - 1) * step] per axis.  Sample: gpis_dfield_sample's interpolant d and its
 * gradient at the fp32 world point; inside iff d < 0 (the field's level is zero by construction; there is no level and no
 * variance gate: max_var was applied when the field was built).  A NaN sample (outside the lattice: after the clip only at the
 * box's faces, through rounding) counts as outside / unknown and advances the ray by min_step.  Step: clamp(|d| - slack * step,
 * min_step, max_step) of arc length, slack in lattice steps.  On lattice points the stored |d| exceeds the distance to the
 * nearest anchor by at most 2 steps (§7e) and the interpolant adds at most sqrt(3)/2 steps (sqrt(2)/2 in 2-D), so with
 * slack >= 2.87 an unclamped step never exceeds the distance to the nearest anchor.  Anchors sample the surface once per crossed
 * lattice edge: this bounds tunnelling at the field's own resolution, not below it, and a step clamped up to min_step can pass
 * through anything thinner than min_step.  d = +-inf (a field without sites) steps max_step and ends as a miss.
 * Output per ray: depth (z / r), record [d, grad(dim)] at the reported point -- the gradient is the surface normal the field
 * sees -- and status (0 hit, 1 left the clipped interval, 2 max_steps samples); no hit: NaN.  One fused kernel marches every ray
 * from set-up to output in one thread; nothing is written per sample; the counters (samples, hits, the largest sample count of
 * a ray) come from a fixed-order reduction.  Same bits on every run, stream and thread-to-pixel mapping.
 * map: may be NULL; it is read only for what the caller leaves NULL: the camera (cam NULL) in 3-D, the sensor offset (off2
 * NULL) in 2-D.  A field from gpis_dfield_from_grid renders without a map.  The renderer moves to the field's device;
 * hip_stream NULL: the field's own stream.  The result is read through gpis_render_get / _device / _info.
 * Errors: a NULL field, renderer or pose, cam / off2 NULL without a map, a bad camera, a non-finite pose or beam angle, a field of
 * another dim, non-finite tnear / tfar, tnear < 0, tnear >= tfar, min_step <= 0, non-finite or > max_step, a NaN max_step, a
 * negative or non-finite slack, refine outside [0, 64], max_steps < 1 -> GPIS_ERR_ARG; a field without a result ->
 * GPIS_ERR_STATE; more than 2^26 rays -> GPIS_ERR_LIMIT: all with the previous result untouched.  Any other failure leaves no
 * result. */
typedef struct gpis_render_field_opts {
    float tnear, tfar;          /* ray interval: depth (3-D) / range (2-D) */
    float min_step, max_step;   /* clamp of |d| - slack * step as the arc-length step; max_step may be +inf */
    float slack;                /* lattice steps taken off |d| */
    int refine;                 /* bisection rounds */
    int max_steps;              /* samples per ray */
} gpis_render_field_opts;
/* defaults for a field of lattice step `step`: tnear, tfar and max_steps as gpis_render_default_opts; min_step = step / 2 (the
 * field holds no feature thinner than a cell), max_step +inf, slack 3, refine 8.  A step that is not finite and positive ->
 * GPIS_ERR_ARG */
int   gpis_render_field_default_opts(int dim, float step, gpis_render_field_opts* opts);
/* thread-to-pixel mapping of the 3-D field kernel (test hook: the results do not depend on it): 1 = a wavefront owns an 8 x 8
 * pixel tile (the default), 0 = 64 consecutive rays of the column-major image */
int   gpis_render_set_field_tiles(void* render, int on);
/* depth [W*H], record [W*H][4], status [W*H].  opts NULL: the defaults for the field's step */
int   gpis3_render_depth_field(void* map, void* df, void* render, const gpis_cam* cam, const float* pose12,
                               const gpis_render_field_opts* opts, void* hip_stream);
/* range [n], record [n][3], status [n].  off2: the sensor offset (x, y) in the laser frame, NULL = the map's.  More than 2^26
 * beams -> GPIS_ERR_LIMIT before thetas is read */
int   gpis2_render_scan_field(void* map, void* df, void* render, const float* thetas, int n, const float* off2,
                              const float* pose6, const gpis_render_field_opts* opts, void* hip_stream);

/* ---- planning: shortest collision-free paths through a distance field on the device ----------------------
 * A navigation function over the free space of the field's lattice (dim, n, origin, step; index p = (k ny + j) nx + i; world
 * point origin + (float)i * step), in float32 without FMA.  Free iff dist[p] >= clearance (+inf is free, negative values and
 * -inf are not); unknown space was made "outside" when the field was built (§7e) and therefore counts as FREE: the plan is
 * only as good as the field's sign.  Point cost c = 1 + gain * (t * t), t = max(0, margin - (dist - clearance)) / margin
 * (margin 0: c = 1).  Offsets (dx, dy, dz) in {-1, 0, 1}^dim, direction index k = ((dz + 1) 3 + (dy + 1)) 3 + (dx + 1), 13 =
 * stay; connectivity 0: the 4 / 6 axis offsets, 1: all 8 / 26.  A move p -> q = p + o exists iff q is in the lattice and p +
 * every non-empty subset of o's non-zero components is free (no squeezing between blocked corners); its weight is
 * w = (len * step) * (0.5f * (c[p] + c[q])), len = 1, sqrtf(2.f), sqrtf(3.f).  A goal snaps to i = (int)floorf(u + 0.5f),
 * u = (x - origin) / step per axis; one that is outside the lattice, non-finite or not free is dropped.  cost = the greatest
 * solution of cost[p] = min over moves of fl(cost[q] + w) with 0 at the kept goals: +inf where not free or unreachable.  The
 * fixed point does not depend on the order of relaxations, so the bits are those of a float32 Dijkstra, on every run and for
 * every schedule.  policy[p] = 13 at a goal, else the k minimising fl(cost[q] + w) (ties: the smaller cost[q], then the
 * smaller k), 255 where there is none.  No goal kept: the solve succeeds with every cost +inf and every policy 255.
 * The planner owns its buffers (10 B per lattice point, grow-only, reused), copies the lattice geometry and reads dist only
 * during gpis_plan_solve: a finished plan stays valid when the field is recomputed or destroyed.  It moves to the field's
 * device; hip_stream NULL: the field's own stream (gpis_plan_paths: the planner's); every call returns with its work finished.
 * Errors: a NULL plan, field, goals or starts, ngoals < 1, m < 1, a non-finite or negative margin or gain, a non-finite
 * clearance, connectivity outside {0, 1}, max_rounds < 0, max_points < 2, gain > 1e4 (which keeps every w far above an ulp of
 * any reachable cost, so that a policy step always lowers the cost) -> GPIS_ERR_ARG; a field without a result, or paths /
 * getters without a solve -> GPIS_ERR_STATE; more than 2^24 starts -> GPIS_ERR_LIMIT: all with the previous result untouched.
 * max_rounds > 0 exceeded -> GPIS_ERR_LIMIT and no result (0: no cap other than lattice points + 1, which a converging solve
 * cannot reach).  Any other failure leaves no result. */
typedef struct gpis_plan_opts {
    float clearance;            /* free iff dist >= clearance */
    float margin, gain;         /* point cost 1 + gain at contact with the clearance, falling to 1 at clearance + margin */
    int connectivity;           /* 0: axis moves, 1: diagonals too */
    int max_rounds;             /* cap on the outer rounds; 0 = none */
} gpis_plan_opts;
/* clearance 0, margin 4 * step, gain 4, connectivity 1, max_rounds 0 */
int   gpis_plan_default_opts(int dim, float step, gpis_plan_opts* opts);
void* gpis_plan_create(void);                              /* on the current device; NULL without one */
void  gpis_plan_destroy(void* plan);
/* goals: host [ngoals][dim].  opts NULL: the defaults for the field's step */
int   gpis_plan_solve(void* plan, void* df, const float* goals, int ngoals, const gpis_plan_opts* opts, void* hip_stream);
/* out[0..n): 1 if a result is held, dim, n[3], the step, goals given, goals kept, free points, reachable points, outer rounds,
 * tile launches, ms of host wall time in the solve, the largest finite cost (14 values) */
int   gpis_plan_info(void* plan, double* out, int n);
/* host copies, prod(n) each; either may be NULL */
int   gpis_plan_get(void* plan, float* cost, unsigned char* policy);
/* device pointers of the last result, valid until the next solve or gpis_plan_destroy (NULL where there is none) */
int   gpis_plan_device(void* plan, const float** d_cost, const unsigned char** d_policy);
/* Paths from the host starts [m][dim], each snapped like a goal.  Status 1: outside the lattice or non-finite; 2: not free;
 * 3: free but cost +inf (these three give no points); otherwise the policy is followed to a goal and the world point of every
 * lattice point visited is emitted, start and goal included: status 0.  A step whose target does not have a strictly smaller
 * cost, or reaching max_points before the goal, ends the path with status 4, the points so far kept.  The paths are packed
 * back to back at offsets from an exclusive scan of their lengths: the same on every run. */
int   gpis_plan_paths(void* plan, const float* starts, int m, int max_points, void* hip_stream);
int   gpis_plan_path_counts(void* plan, long long* npaths, long long* npoints);
/* off[m + 1], points[off[m]][dim], start_cost[m] (NaN for status 1), status[m]; any may be NULL */
int   gpis_plan_get_paths(void* plan, long long* off, float* points, float* start_cost, unsigned char* status);
/* test hook (the results do not depend on it): outer rounds per read-back of the convergence count (0 = 8, at most 64) and
 * relaxation sweeps of a tile per outer round (0 = 256) */
int   gpis_plan_set_schedule(void* plan, int check_every, int inner_cap);

/* ---- trajectories: planned paths smoothed into clearance-keeping trajectories on the device --------------
 * A batch of m trajectories of N waypoints x_0 .. x_{N-1} (dim 2 or 3, 3 <= N <= 256), x[(t N + i) dim + a]; x_0 and x_{N-1}
 * never move, n = N - 2 interior points.  Everything is float32 without FMA and every sum has one order (tests/traj_ref.py
 * states it in numpy), so the bits are the same on every run, stream and batch composition.
 * Input, either of
 *  - gpis_traj_from_paths: every path Q_0 .. Q_{L-1} of the planner's last gpis_plan_paths resampled by arc length:
 *    s_0 = 0, s_k = s_{k-1} + |Q_k - Q_{k-1}| (serial; the norm is sqrtf of squares summed left to right),
 *    t_i = (float)i * (s_{L-1} / (float)(N - 1)), k = the largest index <= L - 2 with s_k <= t_i, w = (t_i - s_k) / (s_{k+1} -
 *    s_k), x_i = Q_k + w (Q_{k+1} - Q_k); x_0 = Q_0 and x_{N-1} = Q_{L-1} are copies; L = 1: N copies of Q_0.  A path of any
 *    status but 0 gives no input: NaN waypoints, status 2;
 *  - gpis_traj_set: host waypoints [m][N][dim]; a trajectory with a non-finite coordinate has status 2 and is returned untouched.
 * gpis_traj_optimize always starts from the input (it may be called again with other options or another field) and runs up to
 * `iters` iterations on every trajectory with an input, each independent of the others:
 *  1. (d_i, grad_i) = gpis_dfield_sample's interpolant at x_i, e_i = d_i - clearance.  d_i or a gradient component non-finite
 *     (outside the lattice, a field without sites, +-inf corners): q_i = 0 and grad_i is taken as 0 -- unknown space is free,
 *     as for the planner.  Else q_i = 0 if e_i >= margin, (e_i - margin) / margin if e_i >= 0, else -1; the matching point cost
 *     c_i is 0, ((e_i - margin) * (e_i - margin)) / (2.f * margin), or 0.5f * margin - e_i.
 *  2. a_i = (x_i - x_{i-1}) + (x_i - x_{i+1}), g_i = w_smooth * a_i + w_obs * (q_i * grad_i), per coordinate.
 *  3. delta = inverse(tridiag(-1, 2, -1)) g in closed form: delta_i = (sum over ascending j = 1 .. n, from 0.f, of
 *     (float)(min(i, j) * (n + 1 - max(i, j))) * g_j) / (float)(n + 1).
 *  4. r_i = sqrtf of delta_i's squares summed left to right, R = max r_i; kappa = rate if rate * R <= max_move, else
 *     max_move / R; x_i <- x_i - kappa * delta_i.  The max keeps a NaN: finite waypoints whose a_i or metric row overflows
 *     (inf - inf) end as NaN waypoints with status 1, never as "converged".
 *  5. fl(kappa * R) < tol: done, status 0.  After `iters` iterations without that (also iters = 0): status 1.
 * Evaluation (after the loop; alone with iters = 0): length = sum |x_{i+1} - x_i|, smooth = sum |x_{i+1} - x_i|^2, obstacle =
 * sum of c_i over the interior points, min_dist = the smallest finite sampled distance over every waypoint and over the `sub`
 * points x_i + ((float)s / (float)(sub + 1)) * (x_{i+1} - x_i), s = 1 .. sub, of every segment (+inf if none is finite),
 * nonfinite = the number of those samples whose distance is not finite, collides = min_dist < clearance.  Sums: the values
 * padded with 0 to 256, then for h = 128, 64, .., 1: v[k] += v[k + h] for k < h.  A trajectory of status 2 has iterations 0,
 * NaN length, smooth, obstacle and min_dist, nonfinite 0 and collides 0.
 * The optimiser owns its buffers (grow-only, reused), moves to the planner's (from_paths) or the field's (optimize) device
 * with its input, reads dist only during gpis_traj_optimize and returns with its work finished: a result outlives its field
 * and its planner.  hip_stream NULL: the field's own stream.  A new input drops the result.
 * Errors: a NULL handle, planner, field or x, N outside [3, 256], m < 1, dim outside {2, 3}, a field of another dim than the
 * input, iters < 0, sub < 0 or > 16, a non-finite or negative w_smooth, w_obs, rate, max_move or tol, margin <= 0 or
 * non-finite, a non-finite clearance -> GPIS_ERR_ARG; a field without a result, a planner without paths, optimize without an
 * input, getters without a result -> GPIS_ERR_STATE; more than 2^20 trajectories -> GPIS_ERR_LIMIT: all with the previous
 * input and result untouched.  Any other failure leaves no result. */
typedef struct gpis_traj_opts {
    float clearance;            /* a sample collides iff its distance < clearance */
    float margin;               /* the obstacle term acts where distance - clearance < margin; > 0 */
    float w_smooth, w_obs;      /* weights of the smoothness and the obstacle gradient */
    float rate;                 /* step length along the covariant gradient */
    float max_move;             /* trust region: the largest move of a waypoint in one iteration */
    float tol;                  /* stop once the largest move of an iteration falls below */
    int iters;                  /* iteration cap; 0: evaluation alone */
    int sub;                    /* evaluation points inside every segment, 0 .. 16 */
} gpis_traj_opts;
/* clearance 0, margin 3 * step, w_smooth 1, w_obs 0.25 * step, rate 0.02, max_move 0.5 * step, tol 0.01 * step, iters 100,
 * sub 3.  dim outside {2, 3}, a step that is not finite and positive, NULL opts -> GPIS_ERR_ARG.  Needs no device. */
int   gpis_traj_default_opts(int dim, float step, gpis_traj_opts* opts);
void* gpis_traj_create(void);                              /* on the current device; NULL without one */
void  gpis_traj_destroy(void* traj);
/* the input from the planner's last paths, N waypoints each; the planner's data is read during the call only */
int   gpis_traj_from_paths(void* traj, void* plan, int N);
/* the input from host waypoints x[m][N][dim] */
int   gpis_traj_set(void* traj, const float* x, int m, int N, int dim);
/* opts NULL: the defaults for the field's step */
int   gpis_traj_optimize(void* traj, void* df, const gpis_traj_opts* opts, void* hip_stream);
/* out[0..n): 1 if an input is held, 1 if a result is held, m, N, dim, ms of host wall time in the last optimize (6 values) */
int   gpis_traj_info(void* traj, double* out, int n);
/* host copies of the last result: x[m][N][dim], and per trajectory status (0 stopped by tol, 1 iteration cap, 2 no input),
 * iterations used, length, smooth, obstacle, min_dist, nonfinite, collides; any may be NULL */
int   gpis_traj_get(void* traj, float* x, unsigned char* status, int* iterations, float* length, float* smooth, float* obstacle,
                    float* min_dist, int* nonfinite, unsigned char* collides);
/* device pointers of the last result, valid until the next input, optimize or gpis_traj_destroy (NULL where there is none):
 * d_x[m][N][dim]; d_fres[m][4] = length, smooth, obstacle, min_dist; d_ires[m][4] = status, iterations, nonfinite, collides */
int   gpis_traj_device(void* traj, const float** d_x, const float** d_fres, const int** d_ires);

/* ---- timing: speeds and times on a trajectory handle's last result, control sequences, the controller's seed --
 * The stage between the trajectories above and the sampling controller below.  (The entries are gpis_timing_*: the trajectory
 * and controller sections keep their sets of entries.)  tests/timing_ref.py states every bit in numpy.
 * gpis_timing_time works on the handle's last result (gpis_traj_optimize; iters = 0 is the cheap way to one); every trajectory
 * of result status 0 or 1 is timed on its own, float32 without FMA, one order per sum:
 *  - ds_i = |x_{i+1} - x_i| (sqrtf of squares summed left to right), S_0 = 0, S_i = S_{i-1} + ds_{i-1} ascending.
 *  - Curvature at interior waypoints, a = x_i - x_{i-1}, b = x_{i+1} - x_i, c = x_{i+1} - x_{i-1}: kappa_i = (2.f * |a x b|) /
 *    ((|a| * |b|) * |c|); a x b = |(a_0 * b_1) - (a_1 * b_0)| in 2-D, the norm of ((a_1 b_2) - (a_2 b_1), (a_2 b_0) - (a_0 b_2),
 *    (a_0 b_1) - (a_1 b_0)) in 3-D; kappa_i = 0 where the denominator is 0 and at both ends.
 *  - Slow-down, with a field and slow_dist > 0: d = gpis_dfield_sample's interpolant at x_i; d not finite: no limit (unknown
 *    space is free); e = d - clearance <= 0: v_min; else v_min + (v_max - v_min) * min(e / slow_dist, 1).
 *  - L_i, the limit on the squared speed: v_max * v_max (code 0); where kappa_i != 0: a_lat / kappa_i if a_lat > 0 (1),
 *    (w_max / kappa_i) squared if w_max > 0 (2); the slow-down speed squared (3); each replaces L_i only where strictly
 *    smaller, in this order.  An interior L_i < v_min * v_min becomes v_min * v_min (4).  Then L_0 takes v_start * v_start and
 *    L_{N-1} takes v_end * v_end where strictly smaller (5).
 *  - u_i = min over j of L_j + (2.f * a_max) * (S_i - S_j) for j < i (6), L_i, L_j + (2.f * d_max) * (S_j - S_i) for j > i (7);
 *    v_i = sqrtf(u_i).  The limiter byte is L_i's code unless a cone is strictly below L_i; 6 unless a braking cone is strictly
 *    below every acceleration cone.
 *  - dt_i = 0 where ds_i = 0, else (2.f * ds_i) / (v_i + v_{i+1}); t_0 = 0, t_{i+1} = t_i + dt_i ascending.
 *  - Timing status 0; 3 where some dt_i is not finite (a positive segment between two zero speeds; the times stay as computed);
 *    2 for a trajectory without input: NaN v, t, duration, max_speed, max_curvature, limiter bytes and counts 0.
 *  - duration = t_{N-1}, max_speed = max v_i, max_curvature = max kappa_i, limiter_counts[c] = waypoints of limiter code c.
 * gpis_timing_controls and gpis_timing_follow are double, left to right, nothing contracted, IEEE / and sqrt, on the float32 x, v,
 * t cast to double.  Per trajectory of timing status 0 and k = 0 .. T, tau_k = t0 + (double)k * dt:
 *  - p_k = x_{N-1} if tau_k >= t_{N-1}; else i = the largest index <= N - 2 with t_i <= tau_k, h = t_{i+1} - t_i, e = tau_k - t_i,
 *    acc = (v_{i+1} - v_i) / h, s = v_i * e + ((0.5 * acc) * e) * e, ds_i = sqrt of the squares of x_{i+1} - x_i summed left to
 *    right, w = min(max(s / ds_i, 0), 1), p_k = x_i + w * (x_{i+1} - x_i).
 *  - D_k = p_{k+1} - p_k, n_k = sqrt(Dx * Dx + Dy * Dy); step k moves iff n_k > min_move; h_k = (Dx / n, Dy / n) of the latest
 *    moving step <= k, of the first moving step where there is none before, (1, 0) without a moving step; h_T = h_{T-1}.
 *  - With (c, s) = h_k and (c', s') = h_{k+1}: dim 2: U_k = (v, w), v = (c * Dx + s * Dy) / dt; dim 3: U_k = (vx, vy, vz, w) =
 *    ((c * Dx + s * Dy) / dt, ((-s) * Dx + c * Dy) / dt, Dz / dt).  num = c * s' - s * c', den = 1 + (c * c' + s * s');
 *    den <= 0: w = +-w_limit by the sign of num (num >= 0: +), 0 with w_limit = 0, counted as clamped; else
 *    w = (num / den) / (0.5 * dt), with w_limit > 0 limited to +-w_limit (counted).
 *  - heading0 = h_0, p0 = p_0: the sequence is for a robot at p0 facing heading0.  Timing status 2 or 3: zero controls,
 *    heading0 (1, 0), p0 = x_0, clamped 0.
 * gpis_timing_follow computes the sequence of trajectory `index` with the controller's T straight into the controller's nominal
 * sequence (what gpis_mppi_set_nominal sets, and nothing else of its state), on the controller's stream.
 * Errors: a NULL handle or opts; a non-finite option; v_max, v_min, a_max or d_max <= 0; v_min > v_max; a negative a_lat, w_max,
 * v_start, v_end or slow_dist; a field of another dim or device; dt <= 0, T outside [1, 256], t0 < 0, w_limit < 0, min_move < 0
 * or any of them non-finite; a controller of another dim or device; index outside [0, m) -> GPIS_ERR_ARG.  No result on the
 * handle (time), no timing (get, controls, follow), a field without a result, a controller that is not initialised, a
 * trajectory whose timing status is not 0 (follow) -> GPIS_ERR_STATE.  All before anything is written: the previous timing,
 * result and nominal sequence stay.  A new input or gpis_traj_optimize drops the timing with the result. */
typedef struct gpis_traj_timing_opts {
    float v_max;                /* speed limit; > 0 */
    float v_min;                /* the speed curvature and clearance may slow down to; 0 < v_min <= v_max */
    float a_max, d_max;         /* acceleration and braking limits along the path; > 0 */
    float a_lat;                /* lateral acceleration limit; 0: off */
    float w_max;                /* yaw rate limit; 0: off */
    float v_start, v_end;       /* speeds at the two ends; >= 0 */
    float clearance;            /* the distance at which the slow-down reaches v_min */
    float slow_dist;            /* the slow-down acts where distance - clearance < slow_dist; 0: off */
} gpis_traj_timing_opts;
/* v_max 1, v_min 0.05, a_max 0.5, d_max 0.5, a_lat 0.5, w_max 1, v_start 0, v_end 0, clearance step, slow_dist 4 * step.
 * dim outside {2, 3}, a step that is not finite and positive, NULL opts -> GPIS_ERR_ARG.  Needs no device. */
int   gpis_timing_default_opts(int dim, float step, gpis_traj_timing_opts* opts);
/* df NULL: no slow-down; hip_stream NULL: the field's own stream (the handle's without a field) */
int   gpis_timing_time(void* traj, void* df, const gpis_traj_timing_opts* opts, void* hip_stream);
/* out[0..n): 1 if a timing is held, ms of host wall time in the last gpis_timing_time, in the last gpis_timing_controls */
int   gpis_timing_info(void* traj, double* out, int n);
/* host copies of the last timing: v[m][N], t[m][N], limiter[m][N], and per trajectory status, duration, max_speed,
 * max_curvature, limiter_counts[m][8]; any may be NULL */
int   gpis_timing_get(void* traj, float* v, float* t, unsigned char* limiter, unsigned char* status, float* duration,
                      float* max_speed, float* max_curvature, int* limiter_counts);
/* U[m][T][2 or 4], heading0[m][2], p0[m][dim], clamped[m]; any may be NULL */
int   gpis_timing_controls(void* traj, double dt, int T, double t0, double w_limit, double min_move, double* U, double* heading0,
                           double* p0, int* clamped);
/* heading0_out[2], p0_out[dim]; either may be NULL */
int   gpis_timing_follow(void* mppi, void* traj, int index, double dt, double t0, double w_limit, double min_move,
                         double* heading0_out, double* p0_out);

/* ---- locating: batches of pose hypotheses scored against a distance field on the device -----------------
 * Which of these m poses explains this frame?  The measurement update of Monte-Carlo localisation, the inner loop of
 * correlative scan matching, relocalisation after the tracker lost the pose (status 2): every pose gets the truncated sum of
 * squared field distances of the frame's points, and the poses are ranked by it.  The field tracker (§7f) polishes the best.
 * Points: exactly the tracker's.  3-D: pixels (col, row) = (n stride, m stride), n < W / stride, m < H / stride, column-major,
 * used iff 0.4 < (double)z < 4, local point (u z, v z, z) with u = ((float)col - cx) / fx, v = ((float)row - cy) / fy.  2-D:
 * beams with 0.2 < (double)r < 30 in input order, local ((float)(r c) + off0, (float)(r s) + off1), c, s = cos, sin((double)theta)
 * on the host.  p of them, in that order.
 * Poses: float32, poses12 [m][12] = [t(3), R(9)] column-major, poses6 [m][6] = [t(2), R(4)] (the tracker's layouts).  World
 * point of a local point under a pose: R[a] x + R[3+a] y + R[6+a] z + t[a] (2-D: R[a] x + R[2+a] y + t[a]) left to right in
 * float32 without FMA, R and t straight from the float32 pose: the point the tracker samples when it is handed that pose.
 * Per point: d = gpis_dfield_sample's interpolant at the world point (NaN outside the lattice); e = |(double)d|; the point is
 * an inlier iff d is finite and e <= max_residual; q = e for an inlier, else max_residual; the point adds q * q (double) to
 * the pose's cost and 1 to its inlier count when it is an inlier.  Every other point pays the full truncated price: a pose
 * that throws its points off the lattice ranks last, not first.  The cost is always finite.
 * Per pose, one summation order: slot l (0 <= l < 64) adds the terms of points l, l + 64, l + 128, ... in ascending order from
 * 0.0; the 64 slots are reduced by the halving tree v[k] = v[k] + v[k + h], h = 32 .. 1; cost = v[0].  p = 0: cost 0.0 and 0
 * inliers for every pose.  Poses are independent: a pose has the same bits alone, in any batch, at any batch position, on any
 * stream.
 * Ranking: order = the first min(top_k, m) pose indices by cost ascending, ties by the lower index; top_k = 0: all m.
 * One kernel launch (a wavefront per pose; no atomics), one copy back of 12 bytes per pose, the ranking on the host; every call
 * returns with its work finished.  A locator holds grow-only device buffers (the tracker's set-up: about 30 B per sample,
 * 8 B per pixel; 60 B per pose) reused across calls.
 * map: may be NULL; it is read only for what the caller leaves NULL: the camera (cam NULL) in 3-D, the sensor offset (off2
 * NULL) in 2-D.  The locator moves to the field's device; hip_stream NULL: the field's own stream.
 * Errors: a NULL field, locator, depth, thetas, ranges or poses; cam / off2 NULL without a map; a bad camera (size < 1, fx or fy
 * zero or non-finite); n < 1; m < 1; stride < 1; top_k < 0; a negative, NaN or infinite max_residual; a non-finite beam angle
 * or pose entry; a field of another dim -> GPIS_ERR_ARG.  A field without a result -> GPIS_ERR_STATE.  More than 2^26 pixels /
 * beams or more than 2^24 poses -> GPIS_ERR_LIMIT before anything is allocated (the poses are not read).  All of these leave
 * the previous result untouched; any other failure leaves none. */
typedef struct gpis_locate_opts {
    double max_residual;        /* inlier: |d| <= max_residual; every other point pays max_residual^2 */
    int stride;                 /* 3-D pixel stride of the points; ignored in 2-D (but checked) */
    int top_k;                  /* poses ranked; 0: all */
} gpis_locate_opts;
/* defaults.  3-D: max_residual 0.05, stride 8, top_k 16; 2-D: max_residual 0.5, stride 1 (ignored), top_k 16.  dim outside
 * {2, 3} or NULL opts -> GPIS_ERR_ARG.  Needs no device. */
int   gpis_locate_default_opts(int dim, gpis_locate_opts* opts);
void* gpis_locate_create(void);                            /* on the current device; NULL without one */
void  gpis_locate_destroy(void* locator);
/* depth [W*H] column-major as update(); cam NULL: the map's camera; opts NULL: the defaults */
int   gpis3_locate_depth_field(void* map, void* df, void* locator, const gpis_cam* cam, const float* depth,
                               const float* poses12, int m, const gpis_locate_opts* opts, void* hip_stream);
/* thetas, ranges [n] as update(); off2: the sensor offset (x, y) in the laser frame, NULL = the map's */
int   gpis2_locate_scan_field(void* map, void* df, void* locator, const float* thetas, const float* ranges, int n,
                              const float* off2, const float* poses6, int m, const gpis_locate_opts* opts, void* hip_stream);
/* host copies of the last result (any pointer may be NULL): cost [m], inliers [m], order [ranked]; GPIS_ERR_STATE without one */
int   gpis_locate_get(void* locator, double* cost, int* inliers, int* order);
/* out[0..n): 1 if a result is held, dim, poses, points used, poses ranked, pixels / beams, ms of host wall time of the call */
int   gpis_locate_info(void* locator, double* out, int n);
/* device pointers of the last result, valid until the next call or gpis_locate_destroy: d_cost [m] doubles, d_inliers [m]
 * ints; either may be NULL; GPIS_ERR_STATE without a result */
int   gpis_locate_device(void* locator, void** d_cost, void** d_inliers);

/* ---- Monte-Carlo localisation: a particle filter resident on the device ------------------------------------
 * The loop that keeps a pose belief alive across frames: m <= 2^24 particles in SE(2) / SE(3) live on the device; predict moves
 * them, an update weighs them against a frame with the scorer's cost above, resampling redraws them, and one small block (the
 * estimate's sums, the integer totals, the best index) is all that comes back per step.  tests/pf_ref.py restates every stage
 * in numpy; each stage except one exp has exactly one result, and that exp moves a weight by at most 1 in 2^32.
 * Every floating-point expression below is double, evaluated left to right, not contracted; division and sqrt are IEEE.
 * State: 2-D (x, y, c, s); 3-D (t(3), w, x, y, z), the quaternion of unit norm; per particle an accumulated negative log
 * weight L; per filter a 32-bit tick and the 64-bit seed.  The float32 pose the scorer reads is every component cast from the
 * state: 2-D [x, y, c, s, -s, c]; 3-D [t, R], R column-major from the quaternion: R0 = 1-2(yy+zz), R1 = 2(xy+wz),
 * R2 = 2(xz-wy), R3 = 2(xy-wz), R4 = 1-2(xx+zz), R5 = 2(yz+wx), R6 = 2(xz+wy), R7 = 2(yz-wx), R8 = 1-2(xx+yy).
 * init: the state from float32 poses (the locate layouts): 2-D (t, R[0], R[1]); 3-D t and the quaternion of R by the trace /
 * largest-diagonal branches (tr = R0+R4+R8 > 0: s = 2 sqrt(tr+1), (s/4, (R5-R7)/s, (R6-R2)/s, (R1-R3)/s); else R0 largest:
 * s = 2 sqrt(1+R0-R4-R8), ((R5-R7)/s, s/4, (R3+R1)/s, (R6+R2)/s); else R4 > R8: s = 2 sqrt(1+R4-R0-R8), ((R6-R2)/s, (R3+R1)/s,
 * s/4, (R7+R5)/s); else s = 2 sqrt(1+R8-R0-R4), ((R1-R3)/s, (R6+R2)/s, (R7+R5)/s, s/4)), then divided by its norm.  L = 0,
 * tick = 0, every weight q = 2^32.  The set lives on the device current in the caller; an update needs a field of that device.
 * Random numbers: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85), key
 * (seed & 0xffffffff, seed >> 32), counter (particle slot, tick, k, tag); tag 0 motion noise, tag 1 the resampling offset.
 * Deviate k: S = the integer sum of the eight 16-bit halves of the block, z = (double)(2 S - 8 * 65535) * 0x1.3988e1412ed76p-17:
 * the sum-of-uniforms normal deviate, unit variance, |z| <= 4.899; no transcendental runs on the device.
 * predict: tick += 1; motion is the relative pose in the body frame as double [t, R] (2-D 6, 3-D 12 values; R becomes
 * (cu, su) = (R[0], R[1]) / the quaternion Qu as in init).  2-D, z0..z2: bx = dx + sigma_t[0] z0, by = dy + sigma_t[1] z1,
 * a = (0.5 sigma_r) z2, cn = (1 - a a) / (1 + a a), sn = (a + a) / (1 + a a) (the Cayley map), x += c bx - s by,
 * y += s bx + c by, (c, s) <- ((c, s) (cu, su)) (cn, sn) as complex products, divided by sqrt(c c + s s).  3-D, z0..z5:
 * b[a] = d[a] + sigma_t[a] z_a, t[a] += R[a] b0 + R[3+a] b1 + R[6+a] b2 (R of the quaternion before the step),
 * Q <- (Q (x) Qu) (x) (1, a0, a1, a2), a_k = (0.5 sigma_r) z_{3+k}, divided by its norm.
 * update: cost and inliers per particle = the locate block's, of the float32 poses against the frame's points (bit for bit
 * what gpis*_locate_* returns for gpis_pf_get's poses); L += beta cost; Lmin = min L; q = (uint64)floor(exp(-(L - Lmin)) 2^32);
 * T = sum q, Th = sum (q >> 16), S2 = sum (q >> 16)^2 (integers); neff = (double)Th (double)Th / (double)S2; the estimate =
 * sum (double)q * state column (3-D: every quaternion times +-1 so that its dot product with the quaternion of the
 * lowest-index particle of maximal q is >= 0) in the tracker's reduction order (256-particle segments by a halving tree, the
 * partials zero-padded to a power of two, the same tree), divided by (double)T, the heading / quaternion divided by its
 * norm; then resample iff neff < resample_below * m.
 * resample: tick += 1; C = the inclusive prefix sum of q (the last update's; 2^32 each after init); qs, rem = divmod(T, m);
 * r = ((w0 << 32) | w1) mod qs from the block of counter (0xFFFFFFFF, tick, 0, 1); p_j = j qs + (j rem) div m + r; ancestor
 * a_j = the first i with C_i > p_j; state and pose gathered into the other half of a ping-pong buffer, L = 0.  Equal weights
 * give a_j = j.
 * No kernel waits on another workgroup, no floating-point atomics; results do not depend on schedule or stream.  Every call
 * returns with its work finished.  hip_stream NULL: the filter's own stream.  map: as for locate, read only for what the
 * caller leaves NULL.
 * Errors (each leaves the previous state untouched): a NULL filter, poses, motion, field or frame; dim outside {2, 3}; m < 1; a
 * non-finite pose or motion entry; a negative or non-finite sigma, beta, max_residual or resample_below; stride < 1; a bad
 * camera / beam angle / offset as for locate; a field of another dim or another device -> GPIS_ERR_ARG.  predict, update,
 * resample or get before init, estimate before the first update, a field without a result -> GPIS_ERR_STATE.  More than 2^24
 * particles or 2^26 pixels / beams -> GPIS_ERR_LIMIT before anything is read or allocated. */
typedef struct gpis_pf_opts {
    double max_residual;        /* the scorer's truncation */
    double beta;                /* L += beta * cost */
    double sigma_t[3];          /* motion noise of the translation, body frame (2-D: the first two) */
    double sigma_r;             /* motion noise of the rotation */
    double resample_below;      /* an update resamples iff neff < resample_below * m; 0: never */
    int stride;                 /* 3-D pixel stride of the points; ignored in 2-D (but checked) */
} gpis_pf_opts;
/* defaults.  2-D: max_residual 0.5, beta 2, sigma_t (0.03, 0.03, 0), sigma_r 0.03, resample_below 0.5, stride 1; 3-D:
 * max_residual 0.05, beta 100, sigma_t 0.003 each, sigma_r 0.003, resample_below 0.5, stride 8.  Needs no device. */
int   gpis_pf_default_opts(int dim, gpis_pf_opts* opts);
void* gpis_pf_create(void);                                 /* on the current device; NULL without one */
void  gpis_pf_destroy(void* pf);
/* poses: float32 [m][6] (dim 2) / [m][12] (dim 3) */
int   gpis_pf_init(void* pf, int dim, const float* poses, int m, unsigned long long seed);
/* motion: double [6] / [12]; opts NULL: the defaults (sigma_t and sigma_r are read) */
int   gpis_pf_predict(void* pf, const double* motion, const gpis_pf_opts* opts, void* hip_stream);
int   gpis2_pf_update_scan(void* map, void* df, void* pf, const float* thetas, const float* ranges, int n, const float* off2,
                           const gpis_pf_opts* opts, void* hip_stream);
int   gpis3_pf_update_depth(void* map, void* df, void* pf, const gpis_cam* cam, const float* depth, const gpis_pf_opts* opts,
                            void* hip_stream);
int   gpis_pf_resample(void* pf, void* hip_stream);
/* the last update's estimate (any pointer may be NULL): pose double [6] / [12] = [t, R], neff, totals [3] = T, Th, S2,
 * resampled = 1 if that update resampled */
int   gpis_pf_estimate(void* pf, double* pose, double* neff, unsigned long long* totals, int* resampled);
/* host copies (any pointer may be NULL): state [m][4 / 7], L [m], q [m], cost [m], inliers [m], ancestors [m] of the last
 * resampling (the identity after init), poses float32 [m][6 / 12].  q, cost and inliers are the last update's, in its order */
int   gpis_pf_get(void* pf, double* state, double* L, unsigned long long* q, double* cost, int* inliers, int* ancestors,
                  float* poses);
/* device pointers ptrs[0..n): state, poses, L, q, cost, inliers, ancestors; valid until the next init or resampling (state and
 * poses change halves).  A caller that overwrites the state writes the matching float32 poses too */
int   gpis_pf_device(void* pf, void** ptrs, int n);
/* out[0..n): 1 after init, dim, m, tick, points used, pixels / beams, updates, resamplings, 1 if the last update resampled,
 * neff, ms of host wall time of the last update */
int   gpis_pf_info(void* pf, double* out, int n);

/* ---- sampled model-predictive control against a distance field (MPPI) --------------------------------------
 * The stage that turns "where I am, where the cost-to-go falls, where the obstacles are" into the next velocity command: K
 * noisy control sequences around a nominal one are rolled through a kinematic model for T steps, charged the field's obstacle
 * cost along the way and the planner's cost-to-go (or the distance to a goal point) at the end, and the nominal sequence moves
 * towards their exponentially weighted mean.  The controller lives on the device; a step copies back one block of 88 bytes.
 * tests/mppi_ref.py restates every stage in numpy; each stage except one exp has exactly one result, and that exp moves a
 * weight by at most 1 in 2^32.  Every floating-point expression below is double, evaluated left to right, not contracted;
 * division and sqrt are IEEE; no sin, cos or log runs on the device.  The field sample is float32 exactly as
 * gpis_dfield_sample, taken at the float32 cast of the position.
 * Model, by the field's dim: dim 2: state (x, y, c, s), U = 2 controls (v, w), a unicycle; dim 3: state (x, y, z, c, s), U = 4
 * controls (vx, vy, vz, w), body-frame velocity and yaw rate about z.
 * State of the controller: the nominal sequence Ubar[T][U] (zero after init), a 32-bit tick (0 after init), the 64-bit seed,
 * 1 <= K <= 65536 rollouts, 1 <= T <= 256 steps.
 * Noise: the particle filter's generator and deviate (above) on the counter (k, tick, t * U + u, 2): tag 2; tags 0 and 1 stay
 * the filter's.  Rollout 0 has z = 0 throughout: it is the nominal sequence itself.
 * step: tick += 1; the start is pose's translation and (c, s) = (R[0], R[1]) / sqrt(R[0] R[0] + R[1] R[1]).  For rollout k and
 * t = 0 .. T - 1: e = sigma[u] z, v_u = min(max(Ubar[t][u] + e, umin[u]), umax[u]), d_u = v_u - Ubar[t][u].  Translation with
 * the heading from before the step: dim 2: bx = v0 dt, x += c bx, y += s bx; dim 3: bx = v0 dt, by = v1 dt, x += c bx - s by,
 * y += s bx + c by, z += v2 dt.  Heading: a = (0.5 dt) w, cn = (1 - a a) / (1 + a a), sn = (a + a) / (1 + a a), (c, s) <-
 * (c cn - s sn, s cn + c sn), each divided by sqrt(c c + s s).  Stage cost j of d, the sampled distance at the new position:
 * NaN (off the lattice) -> w_off; d < clearance -> w_col and the rollout's hit count += 1; d < clearance + margin -> r =
 * ((clearance + margin) - d) / margin, j = (w_obs r) r; else 0.  Control cost g = gamma * sum over the u with sigma[u] > 0,
 * ascending from 0.0, of (Ubar[t][u] d_u) / (sigma[u] sigma[u]).  J = (J + j) + g.
 * Terminal term with a planner (its last solve on the field's lattice): per axis u_a = the sampler's float32 lattice
 * coordinate with the same inside test, i_a = min((int)floorf(u_a + 0.5f), n_a - 1), G = cost[i]; off the lattice -> J +=
 * w_off; G infinite -> J += w_col; else J += w_goal (double)G.  With a goal point: J += w_goal sqrt(sum_a (p_a - g_a)^2), the
 * sum in axis order.
 * Weights: Jmin = min J; q_k = (uint64)floor(exp(-((J_k - Jmin) / lambda)) 2^32); T_q = sum q, Th = sum (q >> 16), S2 =
 * sum (q >> 16)^2 as integers; neff = (double)Th (double)Th / (double)S2; best = the lowest index of minimal J.
 * Update: S[t][u] = sum_k (double)q_k d_u[k][t] in the tracker's reduction order (256-rollout segments by a halving tree, the
 * partials zero-padded to a power of two, the same tree); Ubar[t][u] = min(max(Ubar[t][u] + S[t][u] / (double)T_q, umin[u]),
 * umax[u]); then the nominal rollout: rollout 0 of the new Ubar by the same code, its T + 1 states, cost and hit count.
 * u0 = the new Ubar[0].  shift: Ubar[t] = Ubar[t + 1], the last row stays, the tick does not change.
 * No kernel waits on another workgroup, no atomics; results do not depend on schedule or stream.  Every call returns with its
 * work finished.  hip_stream NULL: the controller's own stream.
 * Errors (each leaves the previous state untouched): a NULL controller, field, pose or U; dim outside {2, 3}; K < 1 or T < 1; a
 * non-finite pose (the translation, R[0], R[1]; in 3-D the rest of R is not read), goal or U entry, a heading of norm 0; a
 * non-finite option, dt <= 0, lambda <= 0, a negative sigma / weight / margin, umin[u] > umax[u]; a field or planner of another
 * dim, lattice or device; both or neither of planner and goal -> GPIS_ERR_ARG.  step, get, shift, set_nominal or device before
 * init, a field or planner without a result -> GPIS_ERR_STATE.  K > 65536 or T > 256 -> GPIS_ERR_LIMIT before anything is read
 * or allocated. */
typedef struct gpis_mppi_opts {
    double dt;                  /* the model's time step */
    double lambda;              /* temperature of the weights */
    double gamma;               /* weight of the control cost */
    double sigma[4];            /* noise of each control (dim 2: the first two); 0: that control is not sampled */
    double umin[4], umax[4];    /* control limits */
    double clearance, margin;   /* collision below clearance; the obstacle cost's band above it */
    double w_obs, w_col, w_off, w_goal;
} gpis_mppi_opts;
/* defaults for a field of lattice step `step`: dt 0.1, lambda 1, gamma 0.1, clearance step, margin 2 step, w_obs 1, w_col 100,
 * w_off 100, w_goal 1; dim 2: sigma (0.25, 0.5), umin (0, -1), umax (1, 1), the rest 0; dim 3: sigma (0.25, 0.25, 0.25, 0.5),
 * umin -1 and umax 1 each.  Needs no device. */
int   gpis_mppi_default_opts(int dim, float step, gpis_mppi_opts* opts);
void* gpis_mppi_create(void);                               /* on the current device; NULL without one */
void  gpis_mppi_destroy(void* mppi);
int   gpis_mppi_init(void* mppi, int dim, int K, int T, unsigned long long seed);
/* U: double [T][U], finite; replaces the nominal sequence as it is (the next step clamps what it samples, not Ubar) */
int   gpis_mppi_set_nominal(void* mppi, const double* U);
/* pose: double [6] / [12] = [t, R] as gpis_pf_estimate returns it; exactly one of plan (a planner handle) and goal (double
 * [dim]) is not NULL; opts NULL: the defaults for the field's step; u0: double [U] or NULL */
int   gpis_mppi_step(void* mppi, void* df, void* plan, const double* pose, const double* goal, const gpis_mppi_opts* opts, double* u0,
                     void* hip_stream);
int   gpis_mppi_shift(void* mppi);
/* host copies (any pointer may be NULL): U [T][U] the nominal sequence; of the last step (zero before it) J [K], q [K],
 * hits [K], nominal_states [T + 1][dim + 2]; stats [10] = Jmin, best, neff, T_q, Th, S2, rollouts with a hit, the nominal
 * rollout's cost and hit count, 1 after the first step */
int   gpis_mppi_get(void* mppi, double* U, double* J, unsigned long long* q, int* hits, double* nominal_states, double* stats);
/* device pointers ptrs[0..n): U, J, q, hits, nominal_states; U changes halves with every step and shift */
int   gpis_mppi_device(void* mppi, void** ptrs, int n);
/* out[0..n): 1 after init, dim, K, T, tick, steps, 1 after the first step, ms of host wall time of the last step */
int   gpis_mppi_info(void* mppi, double* out, int n);

/* ---- moving obstacles in the controller's rollouts -----------------------------------------------------------
 * Every stage above reads the distance field of the static map.  A set of moving balls tells the sampling controller what the
 * map cannot: n balls, 0 <= n <= 256 (discs in 2-D, spheres in 3-D), each a centre c[dim], a constant velocity v[dim] and a
 * radius r >= 0 in double, and one epoch: the absolute time at which the centres hold.  Ball i at elapsed time e is at
 * c_a + v_a * e per axis.  tests/obst_ref.py states every rule below in numpy; all arithmetic is double, written left to right,
 * nothing contracted, IEEE / and sqrt, and the device's bits are the reference's.
 * gpis_obst_mppi_step is gpis_mppi_step with one more stage-cost term.  E0 = t_now - epoch on the host.  In rollout k at step t,
 * after the state update, at the new position p: e = E0 + ((double)(t + 1) * dt); q_a = p_a - (c_a + v_a * e); s2 = q_0 q_0 +
 * q_1 q_1 [+ q_2 q_2] from the first square; sep_i = sqrt(s2) - r_i; D = the minimum over i ascending, from +inf, by
 * (sep_i < D ? sep_i : D).  j_dyn = w_col' and dyn_hits += 1 if D < clearance'; (w_obs' r) r with r = ((clearance' + margin')
 * - D) / margin' if D < clearance' + margin'; else 0 (the primed values are the set's options; margin' = 0 leaves no band).
 * J = ((J + j) + j_dyn) + g.  The term is charged off the lattice too (j is then w_off); the field's hit count keeps its
 * meaning.  Per rollout: dyn_hits and min_sep, the minimum over t of D from +inf by the same comparison.  The nominal rollout
 * after the update charges the same term (nominal_cost includes it) and reports its own dyn_hits and min_sep.  Weights, update,
 * tick, shift, gpis_timing_follow, gpis_mppi_get and gpis_mppi_device are unchanged.  With obst NULL or an empty set the call
 * is gpis_mppi_step: the same launches, the same bits in every output, the tick included.
 * The device table of a set is read only during the calls that take the set; no consumer keeps a pointer into it, so a set may
 * be changed or destroyed between any two calls.
 * Errors, each before anything is written (the previous set, the controller's tick and sequence stay): a NULL handle, dim
 * outside {2, 3}, n < 0, a non-finite centre, velocity, radius, epoch, t or t_now, a negative radius, a non-finite or negative
 * option; a set of another dim or device than the controller -> GPIS_ERR_ARG; n > 256 -> GPIS_ERR_LIMIT; whatever
 * gpis_mppi_step refuses stays refused. */
typedef struct gpis_obst_opts {
    double clearance, margin;   /* a hit on a ball below clearance (of separation: distance to the centre minus the radius); the band above */
    double w_obs, w_col;
} gpis_obst_opts;
/* clearance step, margin 4 step, w_obs 1, w_col 100.  Needs no device. */
int   gpis_obst_default_opts(int dim, float step, gpis_obst_opts* opts);
void* gpis_obst_create(void);                               /* on the current device; NULL without one.  Empty, all options 0 */
void  gpis_obst_destroy(void* obst);
/* centre, velocity: double [n][dim]; radius: double [n]; n = 0 empties the set (the pointers are not read) */
int   gpis_obst_set(void* obst, int dim, int n, const double* centre, const double* velocity, const double* radius, double epoch);
int   gpis_obst_set_opts(void* obst, const gpis_obst_opts* opts);
/* host copies (any pointer may be NULL) */
int   gpis_obst_get(void* obst, double* centre, double* velocity, double* radius, gpis_obst_opts* opts);
/* out[0..n): 1 after the first set, dim, n, epoch, device */
int   gpis_obst_info(void* obst, double* out, int n);
/* centre_out [n][dim]: the centres at absolute time t, on the host: c_a + v_a * (t - epoch) */
int   gpis_obst_at(void* obst, double t, double* centre_out);
/* obst: a set or NULL; t_now: the absolute time of `pose`; the rest as gpis_mppi_step */
int   gpis_obst_mppi_step(void* mppi, void* df, void* plan, void* obst, double t_now, const double* pose, const double* goal,
                          const gpis_mppi_opts* opts, double* u0, void* hip_stream);
/* of the last step (any pointer may be NULL): dyn_hits [K], min_sep [K]; stats [4] = rollouts with dyn_hits > 0, the nominal
 * rollout's dyn_hits and min_sep, n of that step.  After a step without balls: zeros, +inf and n = 0 */
int   gpis_obst_mppi_get(void* mppi, int* dyn_hits, double* min_sep, double* stats);
/* Timed trajectories (a handle that holds a timing, gpis_timing_time) against a set.  t_begin: the absolute time at which
 * trajectory time 0 happens.  For each trajectory of timing status 0 and k = 0 .. steps: tau_k = t0 + (double)k * dt, p_k by
 * gpis_timing_controls' rule bit for bit (the robot rests at x_{N-1} after the duration), e_k = (t_begin - epoch) + tau_k,
 * o_{i,k} = c_i + v_i * e_k.  For each interval k = 0 .. steps - 1 and ball i, ascending: a = p_k - o_{i,k}; b = (p_{k+1} - p_k)
 * - (o_{i,k+1} - o_{i,k}); bb = sum_a b_a b_a and ab = sum_a a_a b_a in axis order from the first product; s = 0 unless bb > 0,
 * else x = (-ab) / bb, s = (x > 0 ? x : 0), s = (s < 1 ? s : 1); q = a + s * b; sep = sqrt(sum_a q_a q_a) - r_i: the closest
 * approach in continuous time while both bodies move in straight lines between two samples (the controller's model at that dt).
 * Per trajectory [m] (any pointer may be NULL): min_sep, the least sep by a strict comparison from +inf, so that ties go to
 * the smallest (k, i); min_time = tau_k + s * dt; min_obstacle = i; first_hit = the smallest k with some sep < clearance, else
 * -1; collides.  With n = 0: +inf, NaN, -1, -1, 0; with timing status 2 or 3: NaN, NaN, -1, -1, 0.
 * steps outside [1, 4096], dt <= 0, t0 < 0, clearance < 0, a non-finite argument, a NULL handle, a set of another dim or device
 * -> GPIS_ERR_ARG; a handle without a timing -> GPIS_ERR_STATE.  Nothing of the handle's result or timing changes. */
int   gpis_obst_check_timing(void* traj, void* obst, double dt, int steps, double t0, double t_begin, double clearance,
                             double* min_sep, double* min_time, int* min_obstacle, int* first_hit, int* collides);

/* ---- re-timing: schedules that wait for moving balls to pass ---------------------------------------------------
 * gpis_obst_check_timing can say that a timed trajectory collides; gpis_retime_solve makes it hold again by path-velocity
 * decomposition: the geometry and the timing stay, the search is over when to move.  (The entries are gpis_retime_*: the timing,
 * obstacle and trajectory sections keep their sets of entries.)  tests/retime_ref.py states every rule in numpy; the schedule
 * is integers and flags and depends on no order, every separation is gpis_obst_check_timing's expression, operation for
 * operation in double with nothing contracted, and the device's integers and bits are the reference's.
 * For a handle that holds a timing, each trajectory of timing status 0, the options slot (seconds), max_pause P, clearance and
 * press_on, a set of n balls and t_begin (the absolute time at which the schedule starts):
 *  - Own time runs in slots.  A = the least integer a >= 0 with (double)a * slot >= (double)t_{N-1}; pos_a = the timed
 *    position p of gpis_timing_controls at tau = (double)a * slot, a = 0 .. A, bit for bit.  A > 1024: status 4.
 *  - sep(p0, dp, k, i): gpis_obst_check_timing's sep for one interval and ball i with p_k = p0, p_{k+1} - p_k = dp, t0 = 0,
 *    dt = slot: e_k = TB + (double)k * slot, e_{k+1} = TB + (double)(k + 1) * slot, TB = t_begin - epoch.
 *  - Cell (a, p): own slot a after p pauses, at real slot k = a + p.  pause_free[a][p] iff no ball has sep(pos_a, 0, a + p, i)
 *    < clearance; play_free[a][p] iff no ball has sep(pos_a, pos_{a+1} - pos_a, a + p, i) < clearance.  A NaN separation is
 *    not below the clearance, as in the check.
 *  - reach[0][0] = 1; reach[a][p] = (a > 0 and reach[a-1][p] and play_free[a-1][p]) or (p > 0 and reach[a][p-1] and
 *    pause_free[a][p-1]).  p* = the least p <= P with reach[A][p]; none: status 3.
 *  - The schedule: walk back from (A, p*) to (0, 0).  press_on = 0: the play predecessor wherever it is reached and free, else
 *    the pause predecessor (pauses fall as early as the optimum allows: the robot holds back); press_on = 1: the pause
 *    predecessor first (pauses fall as late as allowed).  own[a + p] = a along the walk; own(k) = A for every k > arrive =
 *    A + p*.  first_pause = the least real slot k with own(k + 1) = own(k), k < arrive; -1 without a pause.
 *  - Per trajectory: status (0 clear as timed, 1 re-timed with pauses, 2 no timing (timing status 2 or 3), 3 no schedule within
 *    max_pause, 4 too long for this slot), arrive, pauses = p*, own_slots = A, first_pause, own[1280].  Status 2 and 4: -1 in
 *    all four and in the table; status 3: own_slots = A, -1 elsewhere.  With n = 0: status 0 and own(k) = min(k, A).
 *  - Pauses are instantaneous: the model of §7l commands velocities, and a_max / d_max of the timing are not kept across a pause.
 * Cost: at worst A (P + 1) 2 n separations per trajectory, one workgroup each.
 * gpis_retime_controls is gpis_timing_controls' second stage with dt = slot and, for step k = 0 .. T - 1, the two positions
 * pos_own(k0 + k) and pos_own(k0 + k + 1): a paused step has zero displacement and takes the heading of the latest moving step by the
 * same rule.  A schedule of status >= 2 stands still as an untimed trajectory does.  gpis_retime_follow writes the sequence of
 * trajectory `index` into the controller's nominal sequence as gpis_timing_follow does; the controller is meant to run at
 * dt = slot.  gpis_retime_check gives gpis_obst_check_timing's five outputs with p_k = pos_own(k), k = 0 .. steps, the balls
 * of `obst` at the real slots from the schedule's t_begin and min_time in real time from it; any set of the handle's dim may be
 * checked against a schedule.  Status >= 2 answers as timing status 2 does.  The certificate: with the solve's set and
 * clearance and steps <= arrive, a schedule of status 0 or 1 has collides = 0 and min_sep >= clearance -- the same
 * expressions on the same operands.
 * Errors: a NULL handle, set or opts; slot <= 0, clearance < 0 or either non-finite; max_pause outside [0, 255]; press_on
 * outside {0, 1}; a non-finite t_begin; a set of another dim or device; T outside [1, 256]; k0 outside [0, 2^20]; w_limit < 0,
 * min_move < 0 or non-finite; steps outside [1, 4096]; a controller of another dim or device; index outside [0, m) ->
 * GPIS_ERR_ARG.  A handle without a timing (solve) or without a schedule (the others), a controller that is not initialised,
 * a trajectory whose schedule status is >= 2 (follow) -> GPIS_ERR_STATE.  All before anything is written.  A new input,
 * gpis_traj_optimize or gpis_timing_time drops the schedule with the timing. */
typedef struct gpis_retime_opts {
    double slot;                /* seconds of a slot; > 0 */
    int    max_pause;           /* P: the most pause slots of a schedule; 0 .. 255 */
    double clearance;           /* a cell is free while no separation is below it; >= 0 */
    int    press_on;            /* 0: pauses as early as the optimum allows; 1: as late */
} gpis_retime_opts;
/* slot 0.1, max_pause 63, clearance step, press_on 0.  dim outside {2, 3}, a step that is not finite and positive, NULL opts
 * -> GPIS_ERR_ARG.  Needs no device. */
int   gpis_retime_default_opts(int dim, float step, gpis_retime_opts* opts);
/* hip_stream NULL: the handle's own stream; returns with the schedule finished */
int   gpis_retime_solve(void* traj, void* obst, double t_begin, const gpis_retime_opts* opts, void* hip_stream);
/* host copies of the last schedule (any may be NULL): status, arrive, pauses, own_slots, first_pause [m]; own [m][1280];
 * the options of the solve; info [2] = t_begin, ms of host wall time in the solve */
int   gpis_retime_get(void* traj, int* status, int* arrive, int* pauses, int* own_slots, int* first_pause, int* own,
                      gpis_retime_opts* opts, double* info);
/* U[m][T][2 or 4], heading0[m][2], p0[m][dim], clamped[m]; any may be NULL */
int   gpis_retime_controls(void* traj, int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0,
                           int* clamped);
/* heading0_out[2], p0_out[dim]; either may be NULL */
int   gpis_retime_follow(void* mppi, void* traj, int index, int k0, double w_limit, double min_move, double* heading0_out,
                         double* p0_out);
/* [m] each; any may be NULL */
int   gpis_retime_check(void* traj, void* obst, int steps, double clearance, double* min_sep, double* min_time,
                        int* min_obstacle, int* first_hit, int* collides);

/* ---- the robot's footprint: body balls in pose checks, rollouts and trajectories -----------------------------
 * Every stage above treats the robot as one point with a scalar clearance.  A footprint is m balls fixed to the robot,
 * 0 <= m <= 16 (discs in 2-D, spheres in 3-D), each an offset b[dim] in the body frame (x forward, y left, z up) and a radius
 * rho >= 0 in double.  tests/body_ref.py states every rule below in numpy; all arithmetic is double, written left to right,
 * nothing contracted, IEEE / and sqrt, and the device's bits are the reference's.
 * The body rule.  A state is (p, c, s): the position p[dim] and the heading (c, s), a yaw about z in 3-D (the controller's
 * model).  Ball j sits at w0 = p0 + (c b0 - s b1), w1 = p1 + (s b0 + c b1), w2 = p2 + b2.  Its field sample is
 * gpis_dfield_sample's, bit for bit, at ((float)w0, (float)w1, (float)w2); d_j = (double)sample - rho_j.  D = the minimum over j
 * ascending, from +inf, by (d_j < D ? d_j : D); jmin = the first j that attains it.  If any ball's sample is NaN (off the
 * lattice) the body is off: D = NaN, jmin = -1.  The heading is used as given: callers pass unit headings (the rollouts pass
 * theirs after their own normalisation).  One ball with offset 0 and radius 0 reproduces the point's bits.
 * gpis_body_clearance: a batch of states, host double [n][dim + 2] = (p, c, s) in the layout of gpis_mppi_get's
 * nominal_states, 1 <= n <= 2^24.  Per state D_out and ball_out = jmin; counts[3] = the states with D < clearance, the states
 * off the lattice, the index of the least D (the lowest index on ties; -1 if every state is off): integer totals and a
 * lexicographic minimum by (D, index), no floating-point atomics.  A state has the same bits alone, in any batch and at any
 * batch position.  Any output pointer may be NULL.  hip_stream NULL: the field's own stream.
 * gpis_body_mppi_step is gpis_obst_mppi_step with the stage cost's sampled distance d replaced by D at the new position and the
 * new heading (the one after the step's Cayley update: the state nominal_states records): NaN -> w_off; D < clearance -> w_col
 * and hits += 1; the band is unchanged.  With a non-empty set of moving balls: sep_j = (the least separation of w_j, in double,
 * from the balls at the step's time) - rho_j per body ball j ascending, Dm = their minimum from +inf by the same strict
 * comparison; dyn_hits, min_sep and the nominal rollout's values keep their meaning with that Dm.  The terminal term, the
 * control cost, the weights, the update, the tick, shift and gpis_timing_follow are unchanged; the goal and the cost-to-go stay
 * at the reference point p.  The nominal rollout after the update uses the same rule.  With body NULL or m = 0 the call is
 * gpis_obst_mppi_step, with obst NULL or empty as well it is gpis_mppi_step: the same launches, the same bits in every output,
 * the tick included.  No new per-rollout buffers: the nominal rollout's body clearance is gpis_body_clearance on
 * nominal_states.
 * gpis_body_traj_clearance: the waypoints of a handle's last result (gpis_traj_optimize; float32 x[m][N][dim]).  The heading at
 * waypoint i comes from a horizontal chord, in double from the float32 waypoints: e = x[k+1] - x[k] (the first two components),
 * n2 = e0 e0 + e1 e1, (c, s) = (e0 / sqrt(n2), e1 / sqrt(n2)), with k the smallest index >= min(i, N - 2) and <= N - 2 with
 * n2 > 0; if there is none, the largest index < min(i, N - 2) with n2 > 0; if there is none, (c, s) = (1, 0).  Then the body
 * rule at every waypoint.  Per trajectory [m] (any pointer may be NULL): D_min, the least D by a strict comparison from +inf
 * (ties: the smallest (i, j)); waypoint and ball, where it occurs; collides = 1 if some D < clearance or some waypoint is off
 * the lattice.  Every waypoint off: NaN, -1, -1, 1.  A trajectory of status 2 (no result): NaN, -1, -1, 0.  Nothing of the
 * handle's result or timing changes.
 * The device table [16][4] = (b0, b1, b2, rho) is written by gpis_body_set and read only during the calls that take the
 * footprint; no consumer keeps a pointer into it, so a footprint may be changed or destroyed between any two calls.
 * Errors, each before anything is written: a NULL handle, dim outside {2, 3}, m < 0, a non-finite entry, a negative radius, a
 * non-finite clearance, a non-finite state or a heading of norm 0, a footprint of another dim or device than its consumer ->
 * GPIS_ERR_ARG; m > 16, n > 2^24 -> GPIS_ERR_LIMIT; a footprint with m = 0 in gpis_body_clearance and
 * gpis_body_traj_clearance (there is nothing to check), a field or a handle without a result -> GPIS_ERR_STATE; whatever
 * gpis_obst_mppi_step refuses stays refused. */
void* gpis_body_create(void);                               /* on the current device; NULL without one.  Empty */
void  gpis_body_destroy(void* body);
/* offset: double [m][dim]; radius: double [m]; m = 0 empties the footprint (the pointers are not read) */
int   gpis_body_set(void* body, int dim, int m, const double* offset, const double* radius);
/* host copies (either pointer may be NULL) */
int   gpis_body_get(void* body, double* offset, double* radius);
/* out[0..n): 1 after the first set, dim, m, device */
int   gpis_body_info(void* body, double* out, int n);
int   gpis_body_clearance(void* df, void* body, const double* states, long long n, double clearance, double* D_out, int* ball_out,
                          int* counts, void* hip_stream);
/* body: a footprint or NULL; the rest as gpis_obst_mppi_step */
int   gpis_body_mppi_step(void* mppi, void* df, void* plan, void* body, void* obst, double t_now, const double* pose,
                          const double* goal, const gpis_mppi_opts* opts, double* u0, void* hip_stream);
int   gpis_body_traj_clearance(void* traj, void* df, void* body, double clearance, double* D_min, int* waypoint, int* ball,
                               int* collides);

/* ---- smoothing for the robot's footprint: body balls in the optimiser ----------------------------------------
 * gpis_smooth_body_optimize is gpis_traj_optimize with the obstacle term applied at the balls of a footprint (m >= 1, dim 2 or 3;
 * in 3-D the body turns about z only).  tests/traj_body_ref.py states every rule in numpy.  Everything not named here is
 * gpis_traj_optimize's, bit for bit: the ends fixed, a_i, the metric, R, kappa, the update before the stop test, tol, the status
 * codes, iters = 0, float32 without FMA.  Per iteration, on the current iterate:
 *   headings  waypoint i = 0 .. N-1 gets (c, s) by gpis_body_traj_clearance's chord rule, in double; it owns its chord iff chord
 *             k0 = min(i, N-2) has n2 > 0, nn_i = sqrt(n2) of that chord; the last waypoint shares chord N-2 with waypoint N-2
 *   balls     j ascending: w_j = the body rule's position (double), sampled at its float32 cast: (smp, grad);
 *             d_j = (float)((double)smp - rho_j); e_j = d_j - clearance; q_j = gpis_traj_optimize's q(e_j); a sample whose value
 *             or a gradient component is not finite has q_j = 0 and grad_j = 0
 *   force     f_i = q_0 grad_0, then f_i + q_j grad_j
 *   torque    r_j = ((float)((-s) b0 - c b1), (float)(c b0 - s b1)); tau_i = q_0 (grad_0[0] r_0[0] + grad_0[1] r_0[1]), then
 *             tau_i + q_j (...); the z component of grad_j enters the force only
 *   chord     t_i = (tau_i / (float)nn_i) * (-(float)s, (float)c) if waypoint i owns its chord, else (0, 0);
 *             T_k = t_k for k < N-2, T_{N-2} = t_{N-2} + t_{N-1}
 *   gradient  g_i[a] = w_smooth a_i[a] + w_obs (f_i[a] + w_turn (T_{i-1}[a] - T_i[a])), a < 2, interior i;
 *             g_i[2] = w_smooth a_i[2] + w_obs f_i[2]
 * What is descended: with w_turn = 1, g is the gradient of 1/2 w_smooth sum_k |x_{k+1} - x_k|^2 + w_obs sum_i sum_j c(e_ij) with i
 * over all N waypoints: the balls of the two end waypoints turn with chords 0 and N-2 and so move x_1 and x_{N-2} through t_0 and
 * t_{N-1}.  The reported `obstacle` leaves the two ends out, so it is not that cost's second term; w_turn != 1 weighs the turn
 * term and is the gradient of no cost.
 * The evaluation in the same launch: length, smooth, min_dist, nonfinite, collides are gpis_traj_optimize's (the point's);
 * obstacle is the tree sum over the interior waypoints of (c(e_0), then + c(e_j)) with gpis_traj_optimize's point cost c at the
 * balls of the result; the body result D_min, waypoint, ball, collides is what gpis_body_traj_clearance(traj, df, body,
 * (double)clearance) returns on the result, bit for bit, and gpis_smooth_body_get reads it without a launch.  With the one-ball
 * zero footprint (b = 0, rho = 0) x, status, iterations and the four float results have gpis_traj_optimize's bits for any w_turn.
 * gpis_smooth_body_default_opts: gpis_traj_default_opts with w_obs = 0.25 step / balls (the term is summed over the balls), and
 * w_turn = 1.  opts NULL: those defaults for the footprint's m; gpis_traj_opts keeps its layout.
 * A body result is a result: gpis_traj_get, gpis_traj_device, gpis_timing_*, gpis_obst_check_timing and
 * gpis_body_traj_clearance work on it unchanged; gpis_traj_optimize or a new input drops the body result with the result.
 * gpis_smooth_from_pose_paths: gpis_traj_from_paths on the points of a pose planner's last gpis_pplan_paths (dim 2; the heading
 * indices are not carried over: the body faces along its chord).  A turn in place repeats a point, so s_{k+1} == s_k occurs;
 * there w = 0.  The segment search skips such segments except at the path's end and in a path that only turns.
 * Errors, each before anything is dropped: a NULL handle, a footprint with m = 0, w_turn negative or not finite, balls outside
 * 1 .. 16, a footprint of another dim than the field or the input, a footprint on another device than the field, whatever
 * gpis_traj_optimize / gpis_traj_from_paths refuse as an argument -> GPIS_ERR_ARG; a field without a result, a handle without
 * input, a pose planner without paths, gpis_smooth_body_get on a handle whose last result came without a footprint
 * -> GPIS_ERR_STATE. */
int   gpis_smooth_body_default_opts(int dim, float step, int balls, gpis_traj_opts* opts, float* w_turn);
int   gpis_smooth_body_optimize(void* traj, void* df, void* body, const gpis_traj_opts* opts, float w_turn, void* hip_stream);
/* per trajectory [m] (any pointer may be NULL) */
int   gpis_smooth_body_get(void* traj, double* D_min, int* waypoint, int* ball, int* collides);
int   gpis_smooth_from_pose_paths(void* traj, void* pplan, int N);

/* ---- the footprint in the moving-obstacle check and in re-timing ---------------------------------------------
 * gpis_obst_check_timing and gpis_retime_* certify a timed trajectory for a point.  The entries below do it for a footprint
 * (m >= 1).  tests/body_time_ref.py states every rule in numpy.  All arithmetic is double, left to right, nothing contracted,
 * with IEEE / and sqrt.
 *  - The timed pose.  For a trajectory of timing status 0 and tau >= 0: p(tau) is gpis_timing_controls' timed position, bit for
 *    bit; i(tau) is the segment index that position's bisection ends on (the largest i <= N-2 with t_i <= tau), and N-1 for
 *    tau >= t[N-1]; the heading (c, s)(tau) is gpis_body_traj_clearance's chord rule at waypoint i(tau), in double on the float32
 *    waypoints: the chord is horizontal, searched forward from min(i, N-2), then backward, and with no usable chord the heading
 *    is (1, 0).  The body holds its segment's heading; it turns at knots.
 *  - Ball positions.  w_j(tau) = the body rule's position of ball j at (p, c, s)(tau): w0 = p0 + (c b0 - s b1),
 *    w1 = p1 + (s b0 + c b1), w2 = p2 + b2, in double with no float32 cast.  No field is sampled.
 *  - The separation of one interval.  For the poses at tau_k and tau_{k+1}, body ball j and moving ball i it is
 *    gpis_obst_check_timing's expression with p_k := w_j(tau_k) and p_{k+1} - p_k := w_j(tau_{k+1}) - w_j(tau_k), then
 *    sep = (sqrt(s2) - r_i) - rho_j.  Between two samples a body ball's centre moves on the chord of its arc (an approximation
 *    where the heading turns inside the interval).  With the one-ball zero footprint every output below has the
 *    point call's bits.
 * gpis_timed_body_check is gpis_obst_check_timing with that separation over k, i, j ascending: min_sep is the least sep by a
 * strict comparison from +inf (ties: the smallest (k, i, j)), min_time and min_obstacle as before, min_ball = j, first_hit = the
 * least k with some sep < clearance; a NaN sep is not below the clearance.  n = 0 and untimed rows answer as the point call does,
 * with min_ball = -1.
 * gpis_timed_body_retime is gpis_retime_solve's dynamic programme with pause_free[a][p] iff no (i, j) has sep < clearance with
 * the pose of own slot a held (every ball's displacement 0) and play_free[a][p] iff none has going from the pose of own slot a to
 * that of a + 1, both at real slot a + p.  A, the status codes, p*, the walk with press_on, the own table and n = 0 are
 * gpis_retime_solve's, and the schedule is stored where gpis_retime_solve stores it: gpis_retime_get, gpis_retime_controls and
 * gpis_retime_follow read it unchanged.  gpis_timed_body_info: out[0] = the number of body balls of the last solve (0 after
 * gpis_retime_solve).
 * gpis_timed_body_retime_check is gpis_retime_check with the pose of own(k) at real slot k and the footprint given to it.  The
 * certificate: with the solve's set, footprint and clearance and steps <= arrive, a schedule of status 0 or 1 has collides = 0
 * and min_sep >= clearance.
 * gpis_timed_body_states: the timed poses (p, c, s) as states_out[m][steps + 1][dim + 2] (gpis_body_clearance's layout) at
 * t0 + k dt, or with retimed = 1 at own(k) of the last schedule with dt = its slot (dt and t0 are not read); rows without a
 * timing or a schedule are NaN.  1 <= steps <= 4096.
 * Errors, each before anything is written or dropped: whatever the point forms refuse; a NULL footprint, one with m = 0, one of
 * another dim or on another device than the trajectories -> GPIS_ERR_ARG. */
int   gpis_timed_body_check(void* traj, void* obst, void* body, double dt, int steps, double t0, double t_begin, double clearance,
                             double* min_sep, double* min_time, int* min_obstacle, int* min_ball, int* first_hit, int* collides);
int   gpis_timed_body_retime(void* traj, void* obst, void* body, double t_begin, const gpis_retime_opts* opts, void* hip_stream);
int   gpis_timed_body_info(void* traj, double* out, int n);
int   gpis_timed_body_retime_check(void* traj, void* obst, void* body, int steps, double clearance, double* min_sep, double* min_time,
                             int* min_obstacle, int* min_ball, int* first_hit, int* collides);
int   gpis_timed_body_states(void* traj, double dt, int steps, double t0, int retimed, double* states_out);

/* ---- routes for the robot's footprint: heading layers in the planner ---------------------------------------
 * gpis_plan_solve plans for a point with one scalar clearance; a long narrow robot has no right scalar.  The pose planner is
 * the same solver on the lattice nx x ny x H of poses (x, y, heading) of a 2-D field, H in {8, 16, 32, 64}: state s = (i, j, h)
 * at index (h ny + j) nx + i.  tests/pplan_ref.py states every rule below in numpy; float32 without FMA as in §7h, except the
 * body rule, which is double as in §7r; the device's bits are the reference's.
 * Headings: the caller's table, double [H][2] = (c_h, s_h), used as given (finite, not both 0; nothing here calls a
 * trigonometric function).  Configuration space: D(i, j, h) = the body rule (above) at p = ((double)(ox + (float)i * step),
 * (double)(oy + (float)j * step)) with the heading (c_h, s_h) -- gpis_body_clearance's D of that state, bit for bit; d =
 * (float)D; the state is free iff d >= clearance, so a body with a ball off the lattice (D NaN) is not free, and where the
 * bilinear sampler meets infinite dist values and returns NaN the state is blocked.  c = gpis_plan_solve's point cost on d.
 * Moves are directed.  Translation (p, h) -> (p + o, h), code k = 9 + (dy + 1) 3 + (dx + 1) (the 2-D direction codes of
 * gpis_plan_solve): exists iff bit k - 9 of moves[h] is set (uint16 [H], the caller's), the target is in the lattice and p +
 * every non-empty subset of o's components is free in layer h; weight (len * step) * (0.5f * (c[s] + c[s'])).  Turn (p, h) ->
 * (p, h +- 1 mod H), codes 27 (+1) and 28 (-1): exists iff both states are free; weight turn * (0.5f * (c[s] + c[s'])).
 * cost = the greatest solution of cost[s] = min over moves s -> s' of fl(cost[s'] + w) with 0 at the kept goals: a float32
 * Dijkstra on the reversed graph, the same bits on every run and for every schedule.  Goals: float [g][3] = (x, y, h); x, y snap
 * as in gpis_plan_solve; h = -1 means every free heading at that point, each counted as a kept goal; a goal that is outside,
 * non-finite or not free is dropped.  policy[s] = 13 at a goal, else the code minimising fl(cost[s'] + w) (ties: the smaller
 * cost[s'], then the smaller code), 255 where not free or unreachable.
 * Pose paths: starts float [m][3] = (x, y, h), h = -1 meaning the free heading of least cost at the snapped point (ties: the
 * smaller h; none free: status 2, start cost +inf).  Status codes and the count / scan / write packing are gpis_plan_paths';
 * every state visited is emitted as its world point and its heading index.
 * gpis_pplan_project fills a plain planner handle with the 2-D summary: cost2[p] = min over h of cost[p, h]; heading2[p] = the
 * first h attaining it (255 where cost2 is +inf); c2[p] = the least c over the free headings (0: none); policy2[p] = 13 where
 * cost2 == 0, 255 where it is +inf, else the code 9 .. 17 whose in-lattice neighbour has the least cost2 (ties: the smaller
 * code) -- a neighbour of smaller cost2 always exists, the first translation of the pose path from (p, heading2[p]) leads to
 * one.  gpis_plan_info then reports free = the points with a free heading, reachable and max_cost of the projection, and the
 * pose solve's goals, goals_kept, rounds, tile_launches and solve_ms.  The projected handle is valid exactly as after
 * gpis_plan_solve (gpis_plan_paths, gpis_traj_from_paths, gpis_body_mppi_step take it unchanged) and outlives the pose
 * planner.  The projection is a guide -- a cost-to-go and a walkable descent for consumers that track a point; the pose path is
 * the certificate that the body fits.  Nothing is checked between lattice points or between heading steps: choose H so that
 * the farthest ball moves at most about one lattice step per heading step.
 * The pose planner owns its buffers (9 B per state, grow-only, reused), copies the lattice geometry and both tables, and reads
 * the field and the footprint only during gpis_pplan_solve: a finished plan outlives both.  hip_stream NULL: the field's own
 * stream (gpis_pplan_paths: the pose planner's); every call returns with its work finished.
 * Errors: a NULL handle or array, ngoals < 1, m < 1, max_points < 2, a 3-D field, H outside {8, 16, 32, 64}, a non-finite
 * heading or (0, 0), a move bit other than the 8 translations', a non-finite option, a negative margin or gain, gain > 1e4,
 * turn outside [step / 64, 1e4 step] (which keeps every weight far above half an ulp of any reachable cost), max_rounds < 0, a
 * goal or start heading that is not an integer in -1 .. H - 1, a footprint on another device -> GPIS_ERR_ARG; a footprint with
 * m = 0 or of dimension 3, a field or a handle without a result -> GPIS_ERR_STATE; nx ny H > 2^28, more than 2^24 starts ->
 * GPIS_ERR_LIMIT: all with the previous result untouched.  max_rounds > 0 exceeded -> GPIS_ERR_LIMIT and no result. */
typedef struct gpis_pplan_opts {
    float clearance;            /* free iff (float)D >= clearance */
    float margin, gain;         /* point cost, as gpis_plan_opts */
    float turn;                 /* the length of one heading step, in the units of step */
    int max_rounds;             /* cap on the outer rounds; 0 = none */
} gpis_pplan_opts;
/* clearance 0, margin 4 * step, gain 4, turn step, max_rounds 0.  Needs no device. */
int   gpis_pplan_default_opts(float step, int H, gpis_pplan_opts* opts);
void* gpis_pplan_create(void);                              /* on the current device; NULL without one */
void  gpis_pplan_destroy(void* pplan);
/* headings: double [H][2]; moves: uint16 [H]; goals: host float [ngoals][3].  opts NULL: the defaults for the field's step */
int   gpis_pplan_solve(void* pplan, void* df, void* body, const double* headings, const unsigned short* moves, int H,
                       const float* goals, int ngoals, const gpis_pplan_opts* opts, void* hip_stream);
/* out[0..n): 1 if a result is held, nx, ny, H, the step, goals given, goal states kept, free states, reachable states, outer
 * rounds, tile launches, ms of host wall time in the solve, the largest finite cost, ms of that time in the set-up kernel (14) */
int   gpis_pplan_info(void* pplan, double* out, int n);
/* host copies, nx ny H each; any may be NULL */
int   gpis_pplan_get(void* pplan, float* cost, unsigned char* policy, float* c);
/* device pointers of the last result, valid until the next solve or gpis_pplan_destroy (NULL where there is none) */
int   gpis_pplan_device(void* pplan, const float** d_cost, const unsigned char** d_policy, const float** d_c);
int   gpis_pplan_paths(void* pplan, const float* starts, int m, int max_points, void* hip_stream);
int   gpis_pplan_path_counts(void* pplan, long long* npaths, long long* npoints);
/* off[m + 1], points[off[m]][2], heading[off[m]], start_cost[m] (NaN for status 1), status[m]; any may be NULL */
int   gpis_pplan_get_paths(void* pplan, long long* off, float* points, int* heading, float* start_cost, unsigned char* status);
/* plan: a gpis_plan_create handle; heading2: host [nx ny] or NULL */
int   gpis_pplan_project(void* pplan, void* plan, unsigned char* heading2);
/* test hook, as gpis_plan_set_schedule */
int   gpis_pplan_set_schedule(void* pplan, int check_every, int inner_cap);

/* ---- coverage: which lattice points of a field a sensor has seen as free space, and its frontiers ----------
 * The field knows surfaces only; unknown space is "outside" in it and therefore free to the planner.  A coverage holder keeps one
 * byte per lattice point of a field: 1 once some integrated depth frame or laser scan has looked through that point.  On it:
 * the frontiers (seen, traversable points that border unseen, traversable ones; clustered and summarised) and a copy of the
 * field restricted to seen space, which every consumer of a field takes unchanged.  tests/cover_ref.py states each rule below in
 * numpy; every result is an integer or a double computed in one fixed order, and the device's bits are the reference's.
 * Lattice point i of an axis: origin + (float)i * step in float32.  Local point of a lattice point x under a float32 pose
 * [t, R column-major] (the tracker's layouts): l = R^T (x - t), l[c] = R[dim c] d[0] + R[dim c + 1] d[1] (+ R[dim c + 2] d[2]),
 * d = (double)x - (double)t, left to right in double without FMA.
 * 3-D (gpis3_cover_depth): seen iff l.z > 0, the nearest pixel (floor(fx l.x / l.z + cx + 0.5), floor(fy l.y / l.z + cy + 0.5))
 * lies inside the image, its depth d is valid (0.4 < (double)d < 4, the tracker's window) and l.z < d - back_off.  Every pixel
 * counts.  2-D (gpis2_cover_scan): the host keeps the valid beams (0.2 < (double)r < 30) with their host-double directions
 * (c, s), sorts them stably by the diamond pseudo-angle q = 1 - c / (|c| + |s|) for s >= 0, else 3 + c / (|c| + |s|), and keeps
 * per sector k -> k + 1 (the last wraps to the first) lim = min(r_k, r_k+1) - back_off and narrow = (dq < 2) and (c_k c_k+1 +
 * s_k s_k+1 >= cos(max_gap)).  The device takes l = R^T (x - t) - off2 and its sector, the last k with q_k <= q(l) (none: the
 * wrapping one); seen iff that sector is narrow, lim > 0 and l.l < lim^2.  Fewer than two valid beams: nothing is seen;
 * l.l == 0: seen when two or more valid beams exist.  A beam without a return leaves a wide sector, hence unseen space.
 * One thread per lattice point reads its own byte and writes its own byte: no atomics, the same bits on every run.
 * Frontiers (gpis_cover_frontiers): p is a frontier point iff seen[p] and dist[p] >= clearance and some axis neighbour q inside
 * the lattice has !seen[q] and dist[q] >= clearance (float32 compares: NaN fails).  Their lattice indices come out ascending;
 * connected components under full connectivity (8 / 26 neighbours), labelled by their smallest lattice index; per component of
 * at least min_size points, ordered by label: the point count, the integer sums of (i, j, k), the integer bounding box and the
 * representative -- the member nearest the centroid, squared distance (i - sum_i / count)^2 + (j - ..)^2 (+ (k - ..)^2) in double
 * left to right, ties to the smallest index.  Smaller components keep their labels and are dropped from the table.
 * gpis_cover_restrict: df_out gets df_in's lattice and sites, dist_out = seen ? dist_in : unseen_dist; it holds no f grid.
 * The holder owns its buffers (1 B per lattice point; frontiers: 4 B per lattice point and 20 B per frontier point; grow-only,
 * reused) and moves to the field's device; hip_stream NULL: the holder's own stream; every call returns with its work finished.
 * map: may be NULL; it is read only for what the caller leaves NULL (cam / off2), as for locate.
 * Errors: a NULL handle, field, depth, thetas, ranges or pose; cam / off2 NULL without a map; a bad camera; n < 1; a non-finite
 * pose entry or beam angle; back_off negative or non-finite; max_gap outside (0, 90 degrees); clearance <= back_off (every surface
 * would raise a frontier) or non-finite; min_size < 1; max_rounds < 0; a frame of another dim than the lattice; a field of
 * another lattice than the holder's; df_out == df_in; a non-finite unseen_dist -> GPIS_ERR_ARG.  A field without a result, a
 * holder that was never reset, counts / get_frontiers without frontiers -> GPIS_ERR_STATE.  More than 2^26 pixels / beams, or
 * more than max_rounds labelling rounds (the holder then holds no frontiers) -> GPIS_ERR_LIMIT. */
typedef struct gpis_cover_opts {
    float back_off;             /* free space ends this far in front of a measured surface */
    float max_gap;              /* 2-D: the widest angle (radians) between neighbouring valid beams that still closes a sector */
    float clearance;            /* traversable: dist >= clearance */
    int min_size;               /* clusters below it are dropped from the table */
    int max_rounds;             /* labelling rounds; 0: no limit */
} gpis_cover_opts;
/* defaults: back_off step, max_gap 2 degrees, clearance 3 step, min_size 8, max_rounds 0.  Needs no device. */
int   gpis_cover_default_opts(int dim, float step, gpis_cover_opts* opts);
void* gpis_cover_create(void);                              /* on the current device; NULL without one */
void  gpis_cover_destroy(void* cover);
/* the lattice of a field holding a result; seen = 0 everywhere */
int   gpis_cover_reset(void* cover, void* df);
/* the byte mask [prod(n)], x fastest (set: non-zero = seen; n must be the lattice's point count; drops the frontiers) */
int   gpis_cover_set(void* cover, const unsigned char* seen, long long n);
int   gpis_cover_get(void* cover, unsigned char* seen, long long n);
/* device pointer of the mask, valid until gpis_cover_destroy or a reset to a larger lattice (NULL before reset) */
int   gpis_cover_device(void* cover, const unsigned char** d_seen);
/* depth [W*H] column-major as update(); cam NULL: the map's camera; opts NULL: the defaults (back_off is read) */
int   gpis3_cover_depth(void* map, void* cover, const gpis_cam* cam, const float* depth, const float* pose12,
                        const gpis_cover_opts* opts, void* hip_stream);
/* thetas, ranges [n] as update(); off2 NULL: the map's sensor offset (back_off and max_gap are read) */
int   gpis2_cover_scan(void* map, void* cover, const float* thetas, const float* ranges, int n, const float* pose6,
                       const float* off2, const gpis_cover_opts* opts, void* hip_stream);
int   gpis_cover_frontiers(void* cover, void* df, const gpis_cover_opts* opts, void* hip_stream);
/* frontier points, components of any size, clusters in the table */
int   gpis_cover_counts(void* cover, long long* npoints, long long* ncomponents, long long* nclusters);
/* host copies of the last frontiers (any pointer may be NULL): per cluster label [c], count [c], sums [c][3], box [c][6] = min
 * (i, j, k), max (i, j, k), rep [c] (lattice index); per frontier point its lattice index points [m] and label point_label [m] */
int   gpis_cover_get_frontiers(void* cover, int* label, int* count, long long* sums, int* box, int* rep, int* points,
                               int* point_label);
int   gpis_cover_restrict(void* cover, void* df_in, void* df_out, float unseen_dist, void* hip_stream);
/* out[0..n): 1 after reset, dim, n[0], n[1], n[2], step, frames integrated since reset, 1 if frontiers are held, frontier points,
 * components, clusters, labelling rounds, ms of host wall time of the last integrate, of the last frontiers call */
int   gpis_cover_info(void* cover, double* out, int n);

/* ---- scoring candidate viewpoints by the unseen space they would reveal -----------------------------------
 * For each of m candidate poses: what would a sensor there measure of the field (the field renderer's march, §7g), and how many
 * lattice points that are not yet seen would integrating that measurement into the coverage mask turn to seen (the coverage's
 * rule, §7m)?  One call scores the batch on the device; neither the field nor the mask is changed.  tests/view_ref.py composes
 * the two references; every result is an integer and the device's are the reference's.
 * Per pose k: 1. the march of gpis3_render_depth_field / gpis2_render_scan_field with opts->march; the predicted measurement
 * d'[ray] = status == 0 ? depth : miss (float32; status 1 and 2 both miss); hits[k] = rays of status 0.  2. The mask of pose k:
 * the points gpis3_cover_depth / gpis2_cover_scan would see in d' from pose k with back_off (and max_gap), windows (0.4 < d' < 4,
 * 0.2 < r' < 30), per-pose sector table, "fewer than two valid beams" and l.l == 0 rules included.  3. target[p] = !seen[p] and
 * !(dist[p] < min_dist), a float32 compare (a NaN dist counts); gain[k] = the number of targets in the mask of pose k.  With
 * min_dist = -inf, gain[k] is the number of bytes integrating the predicted frame would turn from 0 to 1.  A pose gets the
 * same numbers alone and at any position of any batch.
 * The holder owns its buffers (4 B per pose and ray, 4 B per target, 2-D: 20 B more per pose and beam; grow-only) and moves to the
 * field's device; hip_stream NULL: the field's own stream; every call returns with its work finished.  map: may be NULL; it is
 * read only for a NULL cam / off2.
 * Errors: a NULL view, field, cover, thetas or poses; cam / off2 NULL without a map; a bad camera; n < 1; m < 1; a non-finite
 * pose entry or beam angle; the march's refusals (gpis_render_field_opts); back_off negative or non-finite; max_gap outside
 * (0, 90 degrees); a NaN min_dist; a field of another dim than the sensor -> GPIS_ERR_ARG.  m > 65536 or m x rays > 2^26 ->
 * GPIS_ERR_LIMIT, before the poses are read.  A field without a result, a coverage that was never reset or lies on another
 * lattice than the field's, get / get_predicted without a result -> GPIS_ERR_STATE.  A refused call leaves the
 * previous result readable. */
typedef struct gpis_view_opts {
    gpis_render_field_opts march;   /* the prediction's march */
    float back_off;             /* as gpis_cover_opts */
    float max_gap;              /* as gpis_cover_opts (2-D) */
    float miss;                 /* the measurement of a ray without a predicted return; outside the window, 0 or NaN: it reveals nothing */
    float min_dist;             /* targets: unseen points with !(dist < min_dist); -inf: every unseen point */
} gpis_view_opts;
/* defaults: march gpis_render_field_default_opts(dim, step), back_off step, max_gap 2 degrees, miss = march.tfar - step (the
 * farthest measurement the rule accepts, less one cell), min_dist -inf.  Needs no device. */
int   gpis_view_default_opts(int dim, float step, gpis_view_opts* opts);
void* gpis_view_create(void);                               /* on the current device; NULL without one */
void  gpis_view_destroy(void* view);
/* poses12 [m][12] = [t(3), R(9) column-major]; cam NULL: the map's camera; opts NULL: the defaults for the field's step */
int   gpis3_view_gain_depth(void* map, void* df, void* cover, void* view, const gpis_cam* cam, const float* poses12, int m,
                            const gpis_view_opts* opts, void* hip_stream);
/* thetas [n] as update(); off2 NULL: the map's sensor offset; poses6 [m][6] = [t(2), R(4)] */
int   gpis2_view_gain_scan(void* map, void* df, void* cover, void* view, const float* thetas, int n, const float* off2,
                           const float* poses6, int m, const gpis_view_opts* opts, void* hip_stream);
/* host copies of the last result (either pointer may be NULL); m must be its pose count */
int   gpis_view_get(void* view, long long* gain, int* hits, int m);
/* d' of pose `pose` of the last result; n must be its ray count (3-D: column-major as update()) */
int   gpis_view_get_predicted(void* view, int pose, float* out, long long n);
/* out[0..n): 1 if a result is held, dim, poses, rays per pose, targets, samples of the march, ms of host wall time of the
 * prediction, of the sector tables (2-D), of the target list, of the gather */
int   gpis_view_info(void* view, double* out, int n);

/* ---- moving obstacles detected from a frame's residual against a field ------------------------------------------
 * The stage between "a scan and the field" and the set the controller takes (gpis_obst_*).  tests/detect_ref.py states every rule
 * below in numpy; the device's arrays have its bits.
 *
 * Samples: the tracker's (gpis*_track_*_field: the same validity windows, order, float32 local points and stride), on the sample
 * grid: the beams of a scan, or the W / stride x H / stride strided pixels of a depth frame in column-major order.  x = the
 * sample's world point at the pose cast to float32, d = gpis_dfield_sample's distance there.  A sample is foreign iff d is finite
 * and (double)d >= min_dist and, with a coverage holder, the byte of the lattice point nearest x -- per axis
 * min((int)floorf((x - origin) / step + 0.5f), n - 1) in float32 -- is set.
 * Components: two foreign samples that are neighbours on the grid (2-D: beams k - 1 and k + 1, with no wrap from the last beam to
 * the first; 3-D: the 8 neighbours on the strided grid) are linked iff sum_a e_a e_a <= link * link, e_a = (double)x_a -
 * (double)y_a, summed left to right.  A component's label is its smallest grid index.
 * Per component: count; box = the least and greatest float32 coordinate per axis; centre c_a = 0.5 * ((double)lo_a +
 * (double)hi_a); r2 = the greatest sum_a ((double)x_a - c_a)^2.  Flags: 1 noise (count < min_points), 2 too large (sqrt(r2) >
 * max_radius), 3 dropped for the cap (of the rest the 256 of the largest counts are kept, ties by the lower label), 0 a ball of
 * radius sqrt(r2) + pad.
 * Tracks (host, double): the balls of the previous call at t_prev with velocity, id and age.  Pairs (old i, new j) with
 * |c_j - (c_i + v_i dt)| <= gate + max_speed * dt are taken greedily in ascending (distance, i, j).  Matched: v_raw = (c_j - c_i)
 * / dt, v = alpha v_raw + (1 - alpha) v_i (an old ball of age 0: v_raw whole), the id kept, age + 1.  New: v = 0, a fresh id,
 * age 0.  An unmatched old ball coasts at c_i + v_i dt for up to max_missed calls; coasting balls follow the detected ones in id
 * order while there is room below 256.
 *
 * Errors, all before the previous result is touched: GPIS_ERR_ARG: a NULL handle or array, a non-finite or negative option,
 * alpha outside (0, 1], stride < 1, min_points < 1, a non-finite pose entry or t, a field of another dim, t <= the previous
 * call's with tracks held; GPIS_ERR_STATE: a field without a result, a coverage holder that was never reset or lies on another
 * lattice, getters without a result; GPIS_ERR_LIMIT: more than 2^26 pixels or beams, before anything is read.  max_rounds > 0
 * exceeded: GPIS_ERR_LIMIT, no result is held, the tracks stay; the same holds for GPIS_ERR_HIP (an allocation, a copy or a
 * launch failed once the call was under way).  A frame with no valid or no foreign sample is a result with no
 * balls. */
typedef struct gpis_detect_opts {
    double min_dist;            /* metres; default 2 lattice steps */
    double link;                /* metres; default 3 lattice steps */
    double pad;                 /* metres; default 1 lattice step */
    double max_radius;          /* metres; default 1 */
    double gate;                /* metres; default 4 lattice steps */
    double max_speed;           /* metres per unit of t; default 2 */
    double alpha;               /* default 0.5 */
    int min_points;             /* default 3 */
    int max_missed;             /* default 2 */
    int stride;                 /* 3-D: the pixel stride, default 2; ignored in 2-D */
    int max_rounds;             /* labelling rounds; 0: until converged */
} gpis_detect_opts;
/* a length of k lattice steps is stored as (double)(k * step) with the product in float.  Needs no device. */
int   gpis_detect_default_opts(int dim, float step, gpis_detect_opts* opts);
void* gpis_detect_create(void);                             /* on the current device; NULL without one */
void  gpis_detect_destroy(void* det);
/* check_every: labelling rounds per read-back (1 .. 64; 0 keeps it); profile != 0: synchronise after every stage, so that the
 * stage times of gpis_detect_info are the stages' own.  Neither changes a result. */
int   gpis_detect_set_schedule(void* det, int check_every, int profile);
int   gpis_detect_reset_tracks(void* det);
/* cover: a coverage holder or NULL; cam NULL: the map's camera; pose12 = [t(3), R(9) column-major] in double; t: the absolute time
 * of the frame; opts NULL: the defaults for the field's step */
int   gpis3_detect_depth_field(void* map, void* df, void* det, void* cover, const gpis_cam* cam, const float* depth,
                               const double* pose12, double t, const gpis_detect_opts* opts, void* hip_stream);
/* off2 NULL: the map's sensor offset; pose6 = [t(2), R(4)] in double */
int   gpis2_detect_scan_field(void* map, void* df, void* det, void* cover, const float* thetas, const float* ranges, int n,
                              const float* off2, const double* pose6, double t, const gpis_detect_opts* opts, void* hip_stream);
/* the sizes of the last result: samples of the grid, components, balls */
int   gpis_detect_counts(void* det, long long* grid, long long* components, long long* balls);
/* the balls: centre, velocity [b][dim], radius, count, box [b][6], label, id, age, missed [b] (a coasting ball: count 0, box 0,
 * label -1); any may be NULL */
int   gpis_detect_get_balls(void* det, double* centre, double* velocity, double* radius, int* count, float* box, int* label, int* id,
                            int* age, int* missed);
/* every component in label order: label, count, box [c][6], centre [c][3], r2, flag [c]; any may be NULL */
int   gpis_detect_get_components(void* det, int* label, int* count, float* box, double* centre, double* r2, int* flag);
/* per sample of the grid: label (-1: not foreign or not valid), d (NaN: not valid, or off the lattice), x [g][dim] (0: not
 * valid), the foreign byte; any may be NULL */
int   gpis_detect_get_samples(void* det, int* label, float* dist, float* x, unsigned char* foreign);
/* gpis_obst_set(dim, balls, centre, velocity, radius, epoch = t) with the current balls; the set's options stay */
int   gpis_detect_to_obstacles(void* det, void* obst);
/* out[0..n): 1 if a result is held, dim, grid samples, grid columns, grid rows (3-D), valid samples, foreign samples, components,
 * balls, noise, too large, dropped, labelling rounds, tracks, 1 if tracks are held, t_prev, ms of host wall time of the call, of
 * the set-up, the flags, the compaction, the labelling, the table */
int   gpis_detect_info(void* det, double* out, int n);

/* ---- planning through space and time around moving balls (the contract: tests/tplan_ref.py) ----------------
 * gpis_plan_solve plans through the static field and gpis_retime_solve can only wait on a fixed geometry; gpis_tplan_solve
 * plans on the time-expanded lattice (lattice point x real slot) of a 2-D field, so a route may wait or go another way.
 * Static part: gpis_plan_solve's, bit for bit (point cost c, free iff c > 0, the translations with codes 9 .. 17 without 13,
 * connectivity, no corner cutting, w = (len * step) * (0.5f * (c[p] + c[q])), goals snapped and dropped alike).  Waiting is the
 * move p -> p with code 27, offered after the translations, of weight (wait * step) * c[p] in float32.  Real slots s = 0 .. S
 * (S = horizon), each `slot` seconds long; TB = t_begin - epoch in double; world point P(p) = (double)(origin + (float)i * step).
 * A move p -> q during slot s is clear iff no ball i has sep(P(p), P(q) - P(p), s, i) < dyn_clearance, sep being
 * gpis_obst_check_timing's interval expression with t0 = 0, dt = slot (so e0 = TB + (double)s * slot, e1 = TB + (double)(s + 1) *
 * slot), in double, nothing contracted; a NaN separation is not below the clearance.
 * h[S][p] = 0 at the kept goals, +inf elsewhere; for s = S - 1 .. 0: h[s][p] = 0 at goals, +inf where p is not free, else the
 * minimum of fl(h[s+1][q] + w) over the moves that exist, are clear during slot s and have h[s+1][q] finite.  policy[s][p] = 13 at
 * goals, else the minimising code (ties: the smaller h[s+1][q], then the order offered), 255 without a candidate.  Goals are
 * absorbing.  Layer s depends on layer s + 1 alone: no iteration, and the bits do not depend on the schedule.
 * Storage (grow-only): one policy byte per state, c, the cost of slot 0, two cost layers, and every layer's cost with keep_cost.
 * The handle copies the lattice geometry and the ball table during the solve: a result outlives its field and its set.
 * Errors: NULL handle, field or goals, ngoals < 1, an option outside its range, a non-finite t_begin, a field that is not 2-D,
 * a set of another device or of 3-D balls -> GPIS_ERR_ARG; a field without a result, or readers without a solve / paths ->
 * GPIS_ERR_STATE; nx * ny * (S + 1) > 2^30 (2^28 with keep_cost), more than 2^24 starts -> GPIS_ERR_LIMIT: all with the previous
 * result untouched. */
typedef struct gpis_tplan_opts {
    float clearance, margin, gain;  /* the point cost, as gpis_plan_opts */
    int connectivity;               /* 0: axis moves, 1: diagonals too */
    double slot;                    /* seconds per slot, > 0 */
    int horizon;                    /* S, 1 .. 1024 */
    double dyn_clearance;           /* >= 0: the separation every move keeps from every ball */
    float wait;                     /* 0 .. 1e4: a wait weighs (wait * step) * c[p] */
    int keep_cost;                  /* 1: every layer's cost is kept for gpis_tplan_get */
} gpis_tplan_opts;
/* the planner's clearance 0, margin 4 * step, gain 4, connectivity 1; slot 0.1, horizon 256, dyn_clearance step, wait 0.5,
 * keep_cost 0.  Needs no device. */
int   gpis_tplan_default_opts(float step, gpis_tplan_opts* opts);
/* what gpis_tplan_solve would say to these options on a lattice of nx x ny points (0, 0: the options alone): GPIS_OK,
 * GPIS_ERR_ARG or GPIS_ERR_LIMIT.  Needs no device. */
int   gpis_tplan_check_opts(const gpis_tplan_opts* opts, int nx, int ny);
void* gpis_tplan_create(void);                             /* on the current device; NULL without one */
void  gpis_tplan_destroy(void* tplan);
/* obst NULL or an empty set: no balls.  goals: host [ngoals][2].  opts NULL: the defaults for the field's step */
int   gpis_tplan_solve(void* tplan, void* df, void* obst, const float* goals, int ngoals, double t_begin, const gpis_tplan_opts* opts,
                       void* hip_stream);
/* out[0..n): 1 if a result is held, nx, ny, S, slot, balls, goals given, goals kept, free points, points with a finite cost at
 * slot 0, layer launches, (tile, layer batch, ball) triples the broad phase skipped, ms of host wall time in the solve, the
 * largest finite cost at slot 0, t_begin, 1 if every layer's cost is kept (16 values) */
int   gpis_tplan_info(void* tplan, double* out, int n);
/* host copies: cost0 [nx ny], policy [(S + 1) nx ny], cost_all [(S + 1) nx ny] (GPIS_ERR_STATE without keep_cost), c [nx ny];
 * any may be NULL */
int   gpis_tplan_get(void* tplan, float* cost0, unsigned char* policy, float* cost_all, float* c);
/* device pointers of the last result, valid until the next solve or gpis_tplan_destroy (NULL where there is none) */
int   gpis_tplan_device(void* tplan, const float** d_cost0, const unsigned char** d_policy);
/* Paths from the host starts [m][2], each at slot 0 and snapped like a goal.  Status 1: outside the lattice or non-finite; 2: not
 * free; 3: h[0] = +inf, no arrival within S slots (these give no points); 0: the policy is followed from slot 0 until code 13
 * and one float32 world point is emitted per slot (a wait repeats its point): arrive + 1 points, packed at offsets from a scan. */
int   gpis_tplan_paths(void* tplan, const float* starts, int m, void* hip_stream);
int   gpis_tplan_path_counts(void* tplan, long long* npaths, long long* npoints);
/* off[m + 1], points[off[m]][2], arrive[m] (-1 unless status 0), start_cost[m] (NaN for status 1), status[m]; any may be NULL */
int   gpis_tplan_get_paths(void* tplan, long long* off, float* points, int* arrive, float* start_cost, unsigned char* status);
/* The last paths against any 2-D set at the solve's t_begin and slot: gpis_retime_check's five outputs [m] over the intervals
 * s = 0 .. arrive - 1 of each status-0 path (ties: the smallest (s, i)); a path of another status answers NaN, NaN, -1, -1, 0;
 * n = 0 or arrive = 0 answers +inf, NaN, -1, -1, 0.  With the solve's set and dyn_clearance every status-0 path has collides 0
 * and min_sep >= dyn_clearance: the expressions and the operands are the same. */
int   gpis_tplan_check(void* tplan, void* obst, double clearance, double* min_sep, double* min_time, int* min_obstacle,
                       int* first_hit, int* collides);
/* gpis_retime_controls' stage with dt = slot on the positions P(point at slot min(k0 + k, arrive)), k = 0 .. T (T <= 256):
 * U [m][T][2], heading0 [m][2], p0 [m][2], clamped [m].  A path of status != 0 stands still, p0 the start as given. */
int   gpis_tplan_controls(void* tplan, int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0,
                          int* clamped);
/* test hook (the results do not depend on it): layers per launch (0 = the default: 4 without balls, 1 with them; at most 16) and the broad phase (0 / 1) */
int   gpis_tplan_set_schedule(void* tplan, int layers_per_launch, int cull);

/* ---- planning through space and time for the robot's footprint (the contract: tests/tpplan_ref.py) ----------
 * gpis_tplan_solve plans for a point with one dyn_clearance; gpis_tpplan_solve runs its layer recursion on gpis_pplan_solve's
 * lattice of poses: states (lattice point, heading index h of the caller's table headings[H][2], real slot s = 0 .. S).
 * Static part: gpis_pplan_solve's, bit for bit (the body rule's D at (P(p), (c_h, s_h)), the point cost c on (float)D, free iff
 * c > 0, the directed translations with codes 9 .. 17 without 13 gated by moves[h] and the subset rule per heading layer, the
 * turns 27 (h + 1) and 28 (h - 1) mod H, their weights; goals [g][3] with h = -1 for every free heading, snapped and dropped
 * alike).  Waiting is the move (p, h) -> (p, h) with code 29 and weight (wait * step) * c in float32.  The moves are offered as
 * translations by rising code, 27, 28, 29; every move takes one slot.
 * A move (p, h) -> (q, h') during slot s is clear iff no pair (moving ball i, body ball j) has sep < dyn_clearance: body ball j
 * starts at W0 = P(p) + (c_h b0 - s_h b1, s_h b0 + c_h b1), ends at W1 = the same at (P(q), h'), and sep is
 * gpis_timed_body_check's interval expression with dW = W1 - W0, e0 = TB + (double)s * slot, e1 = TB + (double)(s + 1) * slot,
 * sep = (sqrt(s2) - r_i) - rho_j, in double, nothing contracted; a NaN is not below the clearance.  Between the two ends a
 * ball's centre moves on the chord of its arc.
 * h[S] = 0 at the kept goals, +inf elsewhere; for s = S - 1 .. 0: 0 at goals, +inf where the state is not free, else the minimum
 * of fl(h[s+1][s'] + w) over the moves that exist statically, are clear during slot s and have a finite target.  policy = 13 at
 * goals, else the minimising code (ties: the smaller h[s+1][s'], then the order offered), 255 without a candidate.
 * Storage (grow-only): one policy byte per state, c, the cost of slot 0, two cost layers, and every layer's cost with keep_cost.
 * The handle copies the lattice geometry, the ball table, the footprint and both caller tables during the solve: a result
 * outlives its field, its set and its footprint.
 * Errors: what gpis_pplan_solve and gpis_tplan_solve answer to the same faults (a 3-D field, a set of another device or of 3-D
 * balls, a footprint of another device, a bad table, heading or option -> GPIS_ERR_ARG; a field without a result, an empty or
 * 3-D footprint, readers without a solve / paths -> GPIS_ERR_STATE); nx * ny * H * (S + 1) > 2^30 (2^28 with keep_cost), more
 * than 2^24 starts -> GPIS_ERR_LIMIT: all with the previous result untouched. */
typedef struct gpis_tpplan_opts {
    float clearance, margin, gain, turn;   /* as gpis_pplan_opts */
    double slot;                    /* seconds per slot, > 0 */
    int horizon;                    /* S, 1 .. 1024 */
    double dyn_clearance;           /* >= 0: the separation every body ball keeps from every moving ball */
    float wait;                     /* 0 .. 1e4: a wait weighs (wait * step) * c */
    int keep_cost;                  /* 1: every layer's cost is kept for gpis_tpplan_get */
} gpis_tpplan_opts;
/* the pose planner's clearance 0, margin 4 * step, gain 4, turn step; slot 0.1, horizon 256, dyn_clearance step, wait 0.5,
 * keep_cost 0.  Needs no device. */
int   gpis_tpplan_default_opts(float step, int H, gpis_tpplan_opts* opts);
/* what gpis_tpplan_solve would say to these options with H headings on a lattice of nx x ny points (0, 0: the options alone;
 * turn is only asked to be positive, its range depends on the field's step): GPIS_OK, GPIS_ERR_ARG or GPIS_ERR_LIMIT.  Needs no
 * device. */
int   gpis_tpplan_check_opts(const gpis_tpplan_opts* opts, int H, int nx, int ny);
void* gpis_tpplan_create(void);                            /* on the current device; NULL without one */
void  gpis_tpplan_destroy(void* tpp);
/* obst NULL or an empty set: no balls.  body: a 2-D footprint.  headings [H][2], moves [H], goals [ngoals][3]: host, as
 * gpis_pplan_solve's.  opts NULL: the defaults for the field's step */
int   gpis_tpplan_solve(void* tpp, void* df, void* obst, void* body, const double* headings, const unsigned short* moves, int H,
                        const float* goals, int ngoals, double t_begin, const gpis_tpplan_opts* opts, void* hip_stream);
/* out[0..n): 1 if a result is held, nx, ny, H, S, slot, balls, body balls, goals given, goals kept, free states, states with a
 * finite cost at slot 0, the largest such cost, t_begin, 1 if every layer's cost is kept, layer launches, (tile, layer, ball)
 * triples the broad phase skipped, ms of host wall time in the solve (18 values) */
int   gpis_tpplan_info(void* tpp, double* out, int n);
/* host copies: cost0 [H ny nx], policy [(S + 1) H ny nx], cost_all [(S + 1) H ny nx] (GPIS_ERR_STATE without keep_cost),
 * c [H ny nx]; any may be NULL */
int   gpis_tpplan_get(void* tpp, float* cost0, unsigned char* policy, float* cost_all, float* c);
/* Pose paths from the host starts [m][3] = (x, y, h), each at slot 0 and snapped like a goal; h = -1: the free heading of least
 * slot-0 cost there (ties: the smaller h).  Status 1: outside the lattice or non-finite; 2: no free heading, or the given one
 * not free; 3: cost +inf (these give no entries); 0: the policy is followed from slot 0 until code 13, one float32 world point
 * and one int32 heading index per slot: arrive + 1 entries, packed at offsets from a scan. */
int   gpis_tpplan_paths(void* tpp, const float* starts, int m, void* hip_stream);
int   gpis_tpplan_path_counts(void* tpp, long long* npaths, long long* npoints);
/* off[m + 1], points[off[m]][2], heading[off[m]], arrive[m] (-1 unless status 0), start_cost[m], status[m]; any may be NULL */
int   gpis_tpplan_get_paths(void* tpp, long long* off, float* points, int* heading, int* arrive, float* start_cost,
                            unsigned char* status);
/* The last paths against any 2-D set with any 2-D footprint (body NULL: the solve's) at the solve's t_begin, slot and heading
 * table: gpis_timed_body_check's six outputs [m] over the intervals s = 0 .. arrive - 1 of each status-0 path (ties: the
 * smallest (s, i, j)); min_time = (double)s * slot + sigma * slot.  A path of another status answers NaN, NaN, -1, -1, -1, 0;
 * n = 0 or arrive = 0 answers +inf, NaN, -1, -1, -1, 0.  clearance: >= 0, as gpis_tplan_check's (the solve's dyn_clearance is
 * the caller's to pass).  With the solve's set, footprint and dyn_clearance every status-0 path has collides 0 and min_sep >=
 * dyn_clearance: the expressions and the operands are the solve's own. */
int   gpis_tpplan_check(void* tpp, void* obst, void* body, double clearance, double* min_sep, double* min_time, int* min_obstacle,
                        int* min_ball, int* first_hit, int* collides);
/* gpis_tplan_controls on the paths' points (a turn repeats its point, as a wait does; the heading indices are not tracked) */
int   gpis_tpplan_controls(void* tpp, int T, int k0, double w_limit, double min_move, double* U, double* heading0, double* p0,
                           int* clamped);
/* test hook (the results do not depend on it): the broad phase over the balls (0 / 1) */
int   gpis_tpplan_set_schedule(void* tpp, int cull);

#ifdef __cplusplus
}
#endif
#endif
