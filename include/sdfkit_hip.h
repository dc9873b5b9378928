/* sdfkit_hip.h -- C ABI of libsdfkit_hip.so, the MI355X (gfx950) implementation of
 * SdfKit's hot path  Voxels.SampleSdf -> [Voxels.ClipToBounds] -> MarchingCubes.CreateMesh.
 *
 * The reference (praeclarum/SdfKit, 100 % managed C#) has no FFI boundary of its own;
 * these entry points are what a `[DllImport("sdfkit_hip")]` shim behind the reference's
 * public Sdf / Voxels / MarchingCubes / Mesh API binds.  Each entry
 * point cites the reference interface it replaces (file:line relative to the reference).
 *
 * Conventions: plain pointers and sizes only; every function returns an sdfk_status
 * (0 = OK) and records a thread-local message readable with sdfk_last_error(); the
 * library never retains caller (host) pointers after a call returns; volumes are
 * [nx][ny][nz] row-major (z fastest) exactly like C# `float[nx,ny,nz]` /
 * `Vector3[nx,ny,nz]` (Voxels.cs:8-9).  There is NO CPU fallback: without a HIP device
 * every compute entry point fails with SDFK_ERR_NO_DEVICE.
 */
#ifndef SDFKIT_HIP_H
#define SDFKIT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_abi.py compares `nm -D --defined-only` with the declarations). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define SDFK_ABI_VERSION 6   /* 2: sdfk_jit_stats, sdfk_host_alloc, sdfk_host_free; 3: sdfk_graph_stats; 4: sdfk_set_option, sdfk_dist_*, sdfk_mesh_transform, sdfk_mesh_size_hint;
                                5: SDFK_OPT_ELIDE_VOLUME defaults to 2 (the temporary volume of sdfk_sample_march is not stored); sdfk_init makes a
                                   context per device and per-thread current; sdfk_node_* (several GPUs from one process); sdfk_dist_slab_mesh and exchange
                                   mode 3 (the mesh stays sharded); sdfk_eval_points (SdfEx.Sample);
                                6: SDFK_OPT_COLOR_PASSES; sdfk_dist_gathered refuses a step that brought this rank headers only and sdfk_dist_tune
                                   a session whose exchange mode is 2 or 3 (SDFK_ERR_UNSUPPORTED); gather-to-root has the same who-receives-what on
                                   the host transport as over RCCL; sdfk_host_alloc works in a process whose only contexts are a node's;
                                   entry points added since, existing ones unchanged: sdfk_points_* (KdTree), sdfk_icp_* (IterativeClosestPoint) and
                                   sdfk_trimesh_* (triangle-mesh distance),
                                   sdfk_program_create_bound / sdfk_program_check_bound (programs that read voxel volumes); opcodes
                                   SDFK_OP_SIN .. SDFK_OP_ATAN2 (19-23), accepted by every entry point that takes an op list;
                                   sdfk_points_knn* / sdfk_points_radius_* (KdTree: k nearest, within a radius);
                                   sdfk_points_normals* / sdfk_points_to_volume* (point clouds: normals, signed distance volumes);
                                   sdfk_points_orient_normals* (point clouds: a consistent orientation of the normals);
                                   sdfk_points_voxel_downsample* / sdfk_points_outliers* (point clouds: filters);
                                   sdfk_points_blend_colors* / sdfk_points_to_volume_colors* / sdfk_points_voxel_downsample_colors* (point
                                   clouds: per-point colours);
                                   sdfk_trimesh_components* / sdfk_trimesh_topology* / sdfk_trimesh_select* (triangle meshes: components,
                                   edge census, sub-meshes);
                                   sdfk_points_cluster* / sdfk_points_select* (point clouds: clusters);
                                   sdfk_trimesh_raycast* / sdfk_trimesh_render* (triangle meshes: ray casting) */

typedef enum sdfk_status {
    SDFK_OK = 0,
    SDFK_ERR_INVALID = 1,    /* bad argument */
    SDFK_ERR_NO_DEVICE = 2,  /* no HIP device / sdfk_init not called */
    SDFK_ERR_HIP = 3,        /* a HIP runtime call failed */
    SDFK_ERR_COMPILE = 4,    /* hiprtc failed on a generated SDF kernel */
    SDFK_ERR_NOMEM = 5,
    SDFK_ERR_UNSUPPORTED = 6
} sdfk_status;

/* ---- SDF programs ----------------------------------------------------------
 * Replaces the `Sdf` delegate (Sdf.cs:8) for SDFs that can run on the GPU: the shim
 * lowers an SdfExpr tree (SdfExpr.cs:16-212) or a tagged Sdfs.* factory (Sdf.cs:118-215)
 * to a flat SSA list of scalar float32 operations.  Value id = instruction index.
 * sdfk_program_create validates the list and generates the HIP source of the program's kernels
 * (grid sampler in its row-length instantiations, cell-corner evaluator, ray marcher); each kernel is
 * JIT-compiled with hiprtc -- or loaded from the on-disk code-object cache -- the first time a call
 * needs it (SDFK_ERR_COMPILE is then reported by that call).  The counterpart of
 * SdfExprCompiler.Compile (SdfExpr.cs:225-273).  All arithmetic is IEEE binary32, one rounding
 * per op, no FMA contraction.
 * CONSTANTS ARE ARGUMENTS.  The generated source -- hence the compiled module and its entry in the on-disk cache --
 * depends on the program's STRUCTURE only (opcodes, operand ids, outputs): the `imm` of an SDFK_OP_CONST travels with
 * every launch in the kernel-argument block.  A program with a known structure and other constants (another radius,
 * another period, the next frame of an animation) is created in microseconds and launches the kernels that are already
 * loaded -- in the reference Sdfs.Sphere(radius) is a closure and a new radius costs nothing (Sdf.cs:202-214).  The
 * exceptions are constants one of whose uses the compiler can fold EXACTLY when it sees the value (x * +-1, x / +-1,
 * x / 2^k, x + -0, x - +0, -0 - x): those stay literals and belong to the structure, so that they cost what they always
 * cost; results are bit-identical either way (IEEE-exact foldings only: -ffp-contract=off, no fast-math).  Programs with
 * more than 28 constants keep ALL of them as literals (arguments live in scalar registers: beyond ~30 the sampler spills them,
 * csrc/sample_codegen.h has the measurement) -- such a program is its own structure.  SDFK_OPT_IDLE_PROGRAMS structures stay loaded after their last
 * program has been destroyed. */
typedef enum sdfk_opcode {
    SDFK_OP_CONST = 0,   /* imm (a kernel argument: see above) */
    SDFK_OP_X = 1, SDFK_OP_Y = 2, SDFK_OP_Z = 3,   /* sample point (Voxels.cs:104-106) */
    SDFK_OP_ADD = 4, SDFK_OP_SUB = 5, SDFK_OP_MUL = 6, SDFK_OP_DIV = 7,  /* a ? b */
    SDFK_OP_NEG = 8, SDFK_OP_ABS = 9, SDFK_OP_SQRT = 10, SDFK_OP_FLOOR = 11, /* f(a) */
    SDFK_OP_MIN_SEL = 12, /* (a < b) ? a : b   -- Vector3.Min component */
    SDFK_OP_MAX_SEL = 13, /* (a > b) ? a : b   -- Vector3.Max component */
    SDFK_OP_MIN_IEEE = 14,/* Math.Min / MathF.Min (IEEE 754:2019 minimum) */
    SDFK_OP_MAX_IEEE = 15,/* Math.Max / MathF.Max (IEEE 754:2019 maximum) */
    SDFK_OP_SEL_LT = 16,  /* (a < b) ? c : d   -- SdfExprs.Union (SdfExpr.cs:63-66) */
    /* Reads of a BOUND volume (sdfk_program_create_bound below) at the point (a, b, c); d is a literal, not a value id:
     * d = (slot << 2) | channel, slot 0..7 = the bound volume, channel 0..2 = colour R / G / B, 3 = the distance value.  With
     * D = (Max - Min) / N per axis (float, as Voxels computes DX, Voxels.cs:32-34) and every step ONE f32 operation (no contraction):
     *   SDFK_OP_VOXEL_NEAREST -- the reference's position indexer Voxels[p] (Voxels.cs:48-56): per axis q = (X - Min) / D,
     *     i = (int)q (truncation), CLAMPED to [0, N - 1] -- q <= 0 gives 0, q >= (float)(N - 1) gives N - 1, compared in float
     *     before the conversion.  DEVIATION: where the reference throws IndexOutOfRangeException (a point outside the box) the
     *     GPU form returns the nearest boundary voxel -- an SDF must be total.  A NaN quotient on any axis gives NaN.
     *   SDFK_OP_VOXEL_LINEAR -- trilinear interpolation between the cell centres m + i D, m = Min + 0.5f D (where SampleSdf
     *     samples, Voxels.cs:81): per axis u = (X - m) / D, clamped to [0, N - 1] by compare-select, i0 = min(floor(u), N - 2),
     *     i1 = i0 + 1, f = u - i0 (an axis with N = 1: i0 = i1 = 0, f = 0).  lerp(a, b, f) = a + f (b - a), along x, then y,
     *     then z; the result r is then clamped to [lo, hi] = IEEE minimum / maximum of the 8 corners as
     *     r >= lo ? (r <= hi ? r : hi) : lo -- a NaN corner gives NaN, an overflowing lerp the nearest corner bound.  A NaN
     *     coordinate gives NaN.
     * The interval form (block culling) maps the box of points to a box of indices (both index maps are monotone) and reads
     * its min / max from a min/max pyramid built at bind time; a non-finite voxel makes it unknown. */
    SDFK_OP_VOXEL_NEAREST = 17,
    SDFK_OP_VOXEL_LINEAR = 18,
    /* MathF.Sin / Cos / Exp / Log (f(a)) and MathF.Atan2 (a = y, b = x).  Each is ONE function of float32 to float32, total, and
     * stated exactly (sdfkit_amd/csrc/mathops.h holds the text, which is what the JIT compiles): the argument is widened to
     * binary64, reduced in binary64 (or exactly, in 64-bit integers), a fixed polynomial is evaluated with binary64 + - * / in
     * the stated order (no fma, no hardware approximation, no device library), the result is scaled with ldexp and rounded ONCE
     * to float32.  So numpy reproduces every result bit for bit, and each is faithful (within 1 ulp; nearly always correctly
     * rounded) for every float32.
     *   SIN / COS: q = rint(x (2/pi)), r = ((x - q P1) - q P2) - q P3 (pi/2 in three parts, P1 P2 of 30 bits) for |x| < 2^22;
     *     above, r and q mod 4 from an exact Payne-Hanek reduction against 96 bits of 2/pi (64-bit integer products).  Then
     *     s(r) = r + r^3 (S1 + r^2 (S2 + ... + r^2 S7)), c(r) = 1 + r^2 (C1 + r^2 (C2 + ... + r^2 C8)) (Taylor), and
     *     sin x = s, c, -s, -c for (q & 3) = 0, 1, 2, 3 (cos x: (q + 1) & 3).  sin(+-0) = +-0, cos(+-0) = 1, (+-inf) = NaN.
     *   EXP: k = rint(x log2 e), r = (x - k L1) - k L2 (ln 2 in two parts, L1 of 44 bits), p = 1 + r (1 + r (1/2! + ... r / 13!)),
     *     ldexp(p, k).  x >= 89 gives +inf (overflow), x <= -104 gives +0 (below 2^-150), between: correctly rounded subnormals.
     *     exp(-inf) = +0, exp(+inf) = +inf.
     *   LOG: frexp(x) = m 2^e, m in [sqrt(1/2), sqrt(2)); f = m - 1, s = f / (2 + f), e L1 + (e L2 + (2s + 2s s^2 (1/3 + ... +
     *     s^18 / 21))).  log(+-0) = -inf, log(x < 0) = NaN, log(1) = +0, log(+inf) = +inf.
     *   ATAN2: t = min(|y|, |x|) / max(|y|, |x|), j = rint(8 t), u = (8 t - j) / (8 + t j), a = atan(j/8) + (u + u^3 (A1 + ...
     *     + u^12 A7)); pi/2 - a when |y| > |x|, pi - a when x < 0, negated when y < 0.  C99 Annex F: atan2(+-0, x >= +0) = +-0,
     *     atan2(+-0, x <= -0) = +-(float)pi ((float)pi > pi), atan2(+-inf, +inf) = +-pi/4, atan2(+-inf, -inf) = +-3pi/4,
     *     atan2(y, +-0) = +-pi/2, atan2(y finite, +inf) = +-0, (y finite, -inf) = +-pi.
     * NaN in gives NaN out.  The interval forms (block culling) widen faithful results by one ulp: see csrc/sample_codegen.h. */
    SDFK_OP_SIN = 19, SDFK_OP_COS = 20, SDFK_OP_EXP = 21, SDFK_OP_LOG = 22,
    SDFK_OP_ATAN2 = 23
} sdfk_opcode;
#define SDFK_MAX_VOLUMES 8

typedef struct sdfk_op {
    int32_t opcode;
    int32_t a, b, c, d;  /* operand value ids (unused = -1) */
    float imm;
} sdfk_op;

typedef struct sdfk_program sdfk_program;
typedef struct sdfk_volume sdfk_volume;
typedef struct sdfk_mesh sdfk_mesh;
typedef struct sdfk_march_job sdfk_march_job;

/* ---- lifetime -------------------------------------------------------------- */
int sdfk_abi_version(void);
/* The library's context of HIP device `device` (ordinal) -- created on first use: stream, lanes, pools -- becomes the CALLING THREAD's
 * current context, like hipSetDevice: everything the thread creates afterwards lives on that device.  Idempotent.  A thread that
 * never called sdfk_init works in the context of the first device the process initialised (a host whose calls arrive on pool
 * threads needs nothing else).  Since ABI 5 a second device is not an error: one process may drive several GPUs, one host thread
 * per device (handles are used by threads whose current context is the one they were made in; a mesh's accessors work from any
 * thread).  sdfk_node_open below does exactly that for a whole node.  sdfk_shutdown releases the calling thread's current context. */
int sdfk_init(int device);
void sdfk_shutdown(void);
/* Run on a caller-owned hipStream_t; NULL = the library's own (non-blocking) stream.  NB: the
 * legacy default stream IS the null handle (torch's default stream, for one): passing it selects
 * the library's own stream, which nothing orders against the default stream -- callers that mix
 * their own stream work with library calls create a real stream and pass that
 * (sdfkit_amd/_native.py: bind_torch_stream). */
int sdfk_set_stream(void* hip_stream);
/* Waits for everything the library has queued (the caller's stream and the internal ones). */
int sdfk_synchronize(void);
/* Lane sections.  The calls made between sdfk_lane_begin(lane, ...) and sdfk_lane_end(...) are
 * queued on internal stream `lane` (1..4) instead of the caller's stream, buffers they allocate
 * come from that lane's pool: independent call sequences issued in sections of different lanes
 * overlap on the GPU (what sdfk_sample_march does by itself; a sharded step -- sample a slab,
 * mesh it, pack it -- is such a sequence too).  begin: the lane first waits for
 * `wait_hip_event` (a hipEvent_t the caller recorded, or NULL) -- e.g. "the collective that read
 * this section's output buffer last time has finished".  end(1): the caller's stream waits for
 * everything the section queued, so work the caller queues next (a collective on the packed
 * buffer) sees its results.  Objects created inside a section are used inside sections of the
 * same lane, or after one of their accessors has returned (that waits on the host).  One
 * section at a time per process. */
int sdfk_lane_begin(int32_t lane, void* wait_hip_event);
int sdfk_lane_end(int32_t caller_stream_waits);
const char* sdfk_last_error(void);

/* ---- options ---------------------------------------------------------------
 * Run-time switches of the library (what used to be environment variables read per call).  sdfk_init takes the
 * DEFAULTS from the environment once (SDFK_LANES, SDFK_TOKENS, SDFK_GRAPHS, SDFK_COPY_MODE, SDFK_NO_CORNER_EVAL,
 * SDFK_NO_VCOLOR_EVAL, SDFK_DIST_EXCHANGE, SDFK_NO_CACHE); after that only these calls change or read them. */
typedef enum sdfk_option {
    SDFK_OPT_LANES = 1,         /* internal streams sdfk_sample_march rotates over: 0 (caller's stream), 2, 3 (default), 4 */
    SDFK_OPT_TOKENS = 2,        /* phase tokens, bit 0: sampling kernels of consecutive jobs apart, bit 1: k_vertices apart;
                                   -1 (default) = bit 0 for grids of >= 2^27 voxels */
    SDFK_OPT_GRAPHS = 3,        /* captured launch graphs: 0 never, 1 (default) launch-bound grids, 2 every grid */
    SDFK_OPT_COPY_MODE = 4,     /* device -> caller arrays: 1 (default) bounded pinned ring + thread pool, 0 pre-fault + runtime copy, 2 runtime copy */
    SDFK_OPT_CORNER_EVAL = 5,   /* 1 (default): cell corners of a freshly sampled volume are re-evaluated; 0: gathered */
    SDFK_OPT_VCOLOR_EVAL = 6,   /* 1 (default): vertex colours of a freshly sampled volume are re-evaluated; 0: gathered */
    SDFK_OPT_DIST_EXCHANGE = 7, /* sharded step: 0 (default) ncclAllGather, in place -- the plainest collective; opt-ins: 1 grouped
                                   ncclSend/ncclRecv to every peer (all xGMI links at once), 2 payloads to rank 0 only (headers to all),
                                   3 THE MESH STAYS SHARDED: only the 64-byte headers travel in a step (the counts of every slab on every
                                   rank), the slab payloads stay on their GPUs -- sdfk_dist_slab_mesh hands out a rank's own slab,
                                   sdfk_dist_mesh runs the payload exchange of that one step on demand (collective).  A step is then
                                   no longer bound by what every rank has to receive over xGMI.
                                   sdfk_dist_tune measures 0 against 1 on the node it runs on */
    SDFK_OPT_DIST_LANES = 8,    /* sharded step: internal streams consecutive steps rotate over: 0..3, default 3 (measured: a step on an
                                   8-rank slab of 512^3 takes 82 / 46 / 35 us with 1 / 2 / 3; a fourth shares a hardware queue: 98 us) */
    SDFK_OPT_HW_QUEUES = 9,     /* read-only: GPU_MAX_HW_QUEUES as the process had it when the library came up (0 = unset).  The
                                   HIP runtime maps all streams of a process onto that many in-order hardware queues (default 4);
                                   the library's streams want 8 (sdfk_init in csrc/lib_context.hip says why), and the variable only
                                   counts if it is set before the process's FIRST HIP call: host bindings export it, the
                                   library itself never edits the environment */
    SDFK_OPT_CODE_CACHE = 10,   /* 1 (default): compiled code objects are kept on disk (sdfk_set_cache_dir); 0: off */
    SDFK_OPT_PREFAULT_HUGE = 11,/* 1: whole 2 MiB blocks of a pageable destination are advised MADV_HUGEPAGE before they are first
                                   touched (sdfk_mesh_copy, sdfk_volume_download, sdfk_host_prefault); 0 (default): left as they are
                                   (measured slower where the kernel compacts memory inside the fault) */
    SDFK_OPT_DIST_INDEX16 = 12, /* sharded step, sessions created afterwards: 1 = compact payloads -- the slab's indices travel as uint16 offsets
                                   against one int32 base per 1024 indices (48 -> 36 bytes per vertex of a colourless mesh: what every rank
                                   has to receive from every other rank per step); sdfk_dist_mesh decodes, sdfk_dist_gathered shows the
                                   encoded form.  A slab whose ids do not fit sends the session back to int32 indices (every rank
                                   sees it in the headers).  0 (default): int32 indices, rebased in place by the step */
    SDFK_OPT_STREAM_PLACEMENT = 13, /* at sdfk_init (set it before): 1 (default) = the library measures which of its streams run side by side
                                   on this process's hardware queues / pipes and puts its lanes and the exchange stream where they do not
                                   get in each other's -- or the caller's stream's -- way (about 10 ms); 0 = streams as they come */
    SDFK_OPT_IDLE_LANE = 14,    /* 1 (default): sdfk_sample_march jobs on launch-bound grids (the captured-graph ones) rotate over a FOURTH
                                   internal stream while the caller's stream has nothing queued (hipStreamQuery at the call): that stream
                                   shares the caller's stream's hardware pipe, so it is only used when the caller is not; 0 = never */
    SDFK_OPT_IDLE_PROGRAMS = 15,/* compiled kernel sets are shared by every program of one STRUCTURE (the constants of a program are kernel
                                   arguments, sdfk_program_create); this many structures stay loaded after their last program has been
                                   destroyed (default 32; 0: unloaded at once) -- the next frame of an animation asks for the same one */
    SDFK_OPT_ELIDE_VOLUME = 16, /* The temporary volume of sdfk_sample_march (SdfEx.ToMesh, Sdf.cs:59-63: the Voxels is a local nobody sees),
                                   on grids above the captured-graph limit.  2 (DEFAULT since ABI 5): it is neither stored nor, for the most
                                   part, even evaluated -- 64 x 4 x 4 blocks whose values provably lie on one side of the iso value (the
                                   program evaluated in interval arithmetic over the block: rigorous for the float operations themselves,
                                   no assumption about the SDF) get constant sign words, only the blocks the surface passes through are
                                   evaluated voxel by voxel; cell corners and vertex colours are re-evaluated by the program.  1: every
                                   voxel is evaluated, nothing but the sign bits is stored (4, or 16 with colours, bytes per voxel of HBM
                                   writes less than 0).  0: the volume is evaluated and stored, as the reference does and as the headline
                                   benchmark's step is defined (bench.py sets 0 for its headline).  Meshes are bit-identical in all three.
                                   Never elided: a volume the caller can see (sdfk_sample / sdfk_sample_march_slab / Voxels.SampleSdf:
                                   those always store), step > 1, a NaN iso value, a program one of whose volumes had case-13 sign words
                                   (the dead-cell test of the meshing reads voxels: that job is redone on a stored volume) */
    SDFK_OPT_COLOR_PASSES = 17, /* How Voxels.SampleSdf writes a COLOUR volume (16 B per voxel into two arrays: Voxels.cs:112-120).  One fused pass
                                 * from workgroups that own 8 x rows runs at 0.70-0.75 of the HBM peak even without arithmetic; values (+ sign
                                 * bytes) by that kernel and then the colour array as one linear stream by a second kernel reaches 0.78-0.84
                                 * -- when the program is cheap enough to be evaluated a second time, one voxel per lane.  0 (default): two
                                 * passes for programs of at most 24 operations (one primitive with a constant colour) on grids of at least
                                 * 2^21 voxels, one pass otherwise; 1: always one pass; 2: always two.  Bit-identical results either way. */
    SDFK_OPT_COUNT_BYTES = 18,  /* 1 (default): a sdfk_sample_march job whose fused sampler has just written the sign bytes of its own, stored volume
                                   (step 1, a byte pitch that is a multiple of 8, at most 8192 compaction blocks) counts its active cells straight
                                   from those bytes (k_count_bytes): no sign-word array, no transposer launch.  0: every job regroups the bytes into
                                   words first (k_bits_transpose, k_compact), as all other jobs always do.  Meshes are bit-identical
                                   (an option added since ABI 6; existing keys unchanged) */
    SDFK_OPT_COUNT_ = 19
} sdfk_option;
int sdfk_set_option(int32_t key, int64_t value);
int sdfk_get_option(int32_t key, int64_t* value);
/* Directory of the on-disk code-object cache; NULL = default ($SDFK_CACHE_DIR | $XDG_CACHE_HOME/sdfkit_hip |
 * ~/.cache/sdfkit_hip as the process had them at start-up).  The directory must belong to the calling user and be
 * writable by nobody else, otherwise the cache stays off. */
int sdfk_set_cache_dir(const char* path);

/* out_rgbw = value ids of (colour.X, colour.Y, colour.Z, distance W) -- the Vector4 the
 * delegate writes (Sdf.cs:8).  writes_color = 0 for delegates that only assign `.W`
 * (Sdfs.Sphere/Box/Plane, Sdf.cs:134,153,211): colour stays (0,0,0) (Voxels.cs:88-92). */
int sdfk_program_create(const sdfk_op* ops, int32_t n_ops, const int32_t out_rgbw[4],
                        int32_t writes_color, sdfk_program** out);
/* Generate + hiprtc-compile EVERY kernel of the program for gfx950 without loading (needs no
 * device, never uses the cache): a lowering check the shim can run at build time. */
int sdfk_program_check(const sdfk_op* ops, int32_t n_ops, const int32_t out_rgbw[4], int32_t writes_color);
/* A program that reads volumes (SDFK_OP_VOXEL_NEAREST / SDFK_OP_VOXEL_LINEAR; sdfk_program_create / _check refuse those opcodes with
 * SDFK_ERR_INVALID): the reference's Sdfs.Solid(p => voxels[p]) -- a closure over a Voxels.  volumes[slot] = the volume of slot
 * `slot` (at most SDFK_MAX_VOLUMES).  Refused with SDFK_ERR_INVALID: a slot >= n_volumes, more than 8 volumes, a null, slab
 * (z0 != 0 or nz != nz_global) or elided volume, a volume of another device context, an extent Max - Min <= 0 on any axis, and a
 * COLOUR channel of a volume that has no colour array.
 * SNAPSHOT: the program takes a device copy of each bound volume's Values (and Colors when it reads a colour channel) when it is
 * created, plus a min/max pyramid of every channel it reads (about 8/7 x 8 bytes per 8 voxels per channel): a volume of N voxels
 * costs the program 4 N bytes (+ 12 N with colours) + ~1.15 N bytes per channel read, until the program is destroyed.  Later
 * uploads, samples or a free of the source volume change nothing; a program may be sampled into the very volume it was built
 * from.  WHICH volume is bound is an argument, not structure: another volume with the same slots and channels compiles nothing. */
int sdfk_program_create_bound(const sdfk_op* ops, int32_t n_ops, const int32_t out_rgbw[4], int32_t writes_color,
                              const sdfk_volume* const* volumes, int32_t n_volumes, sdfk_program** out);
/* sdfk_program_check for a program that reads `n_volumes` bound volumes: the offline compile (no device, no volume). */
int sdfk_program_check_bound(const sdfk_op* ops, int32_t n_ops, const int32_t out_rgbw[4], int32_t writes_color, int32_t n_volumes);
/* the generated HIP source of the program's STRUCTURE (constants appear as K.k[i]) */
const char* sdfk_program_source(const sdfk_program* p);
/* JIT bookkeeping of this process.  Compiled code objects are kept on disk (see csrc/lib_jit.hip,
 * "on-disk cache": $SDFK_CACHE_DIR | $XDG_CACHE_HOME/sdfkit_hip | ~/.cache/sdfkit_hip; SDFK_NO_CACHE=1
 * switches it off), so only the first process that sees a program pays for hiprtc -- the counterpart
 * of SdfExprCompiler.Compile (SdfExpr.cs:234-238) paying the expression JIT once per delegate. */
int sdfk_jit_stats(int64_t* n_compiled, int64_t* n_cache_hits, double* compile_ms_total);
void sdfk_program_destroy(sdfk_program* p);

/* ---- Voxels (Voxels.cs:6-65) ------------------------------------------------
 * Device-resident `Values` (+ `Colors` when with_colors != 0).  A *slab* volume holds the
 * voxel planes [z0, z0+nz_local) of a global nx*ny*nz_global grid (multi-GPU Z sharding);
 * sdfk_volume_create is the slab z0 = 0, nz_local = nz. */
int sdfk_volume_create(int32_t nx, int32_t ny, int32_t nz, const float min[3], const float max[3],
                       int32_t with_colors, sdfk_volume** out);
int sdfk_volume_create_slab(int32_t nx, int32_t ny, int32_t nz_global, const float min[3],
                            const float max[3], int32_t z0, int32_t nz_local,
                            int32_t with_colors, sdfk_volume** out);
/* host <-> device copies of Voxels.Values / Voxels.Colors (colors may be NULL) */
int sdfk_volume_upload(sdfk_volume* v, const float* values, const float* colors3);
int sdfk_volume_download(const sdfk_volume* v, float* values, float* colors3);
/* Raw device pointers (the caller may write through them: cached sign bits are dropped and
 * meshes that still depend on the volume are completed first).  The DEVICE arrays pad every z row to
 * sdfk_volume_row_pitch voxels (nz rounded up to a multiple of 4: 16-byte aligned rows for the sampling
 * kernel): voxel (x, y, z) is at ((x * ny + y) * pitch + z), its colour at 3x that.  upload / download
 * convert from / to the dense host layout of Voxels.Values / Voxels.Colors. */
int sdfk_volume_device_ptrs(const sdfk_volume* v, void** values, void** colors3);
int sdfk_volume_row_pitch(const sdfk_volume* v, int32_t* pitch_voxels);
void sdfk_volume_free(sdfk_volume* v);

/* Voxels.SampleSdf(Sdf, batchSize, maxDegreeOfParallelism) (Voxels.cs:72-125): evaluates
 * the program at every cell centre and stores W -> Values, XYZ -> Colors.  batchSize and
 * maxDegreeOfParallelism have no GPU meaning and are not part of the ABI.
 * clip_to_bounds != 0 fuses Voxels.ClipToBounds (SdfEx.ToVoxels, Sdf.cs:49-57). */
int sdfk_sample(const sdfk_program* p, sdfk_volume* v, int32_t clip_to_bounds);
/* Voxels.ClipToBounds (Voxels.cs:133-167) on an existing volume. */
int sdfk_volume_clip_to_bounds(sdfk_volume* v);

/* ---- MarchingCubes.CreateMesh (MarchingCubes.cs:39-92) ----------------------
 * One-shot forms.  The mesh is left on the device; query with sdfk_mesh_*.
 *
 * Completion is DEFERRED: a repeat call for a grid shape sizes its buffers from the previous
 * mesh of that shape, queues every kernel and returns the handle without waiting for the GPU.
 * The first sdfk_mesh_* accessor waits, verifies the size guess and, if it was too small, redoes
 * the job exactly -- the caller never sees a difference except in timing, and errors of the job
 * are reported by that accessor.  The library keeps the source volume's contents alive for that:
 * modifying or freeing a volume (upload, sample, clip, free, device_ptrs) first completes the
 * meshes that still depend on it.  sdfk_mesh_free on an unread mesh does not wait. */
int sdfk_march(const sdfk_volume* v, float iso_value, int32_t step, sdfk_mesh** out);
/* Host-array form: `values`/`colors3` are the managed Voxels.Values / Voxels.Colors arrays
 * pinned by the shim for the duration of the call (colors3 may be NULL = zeros). */
int sdfk_march_host(const float* values, const float* colors3, int32_t nx, int32_t ny, int32_t nz,
                    const float min[3], const float max[3], float iso_value, int32_t step,
                    sdfk_mesh** out);
/* SdfEx.ToMesh (Sdf.cs:59-63): sample (+clip) and mesh without leaving the device.
 * Self-contained jobs: consecutive calls are queued on three internal streams in turn (not on the
 * sdfk_set_stream stream) and overlap on the GPU; their results are safe to use from any stream
 * once an accessor has returned.  sdfk_set_option(SDFK_OPT_LANES, 0) keeps them on the caller's stream.
 * Repeat calls on launch-bound grids (<= 2^24 voxels, step 1): the job of a (program, bounds, grid, clip,
 * iso) is built once per internal stream -- volume, workspace and mesh arrays sized from the previous
 * result of that grid shape -- its kernel launches are captured in a hipGraph, and every later call is
 * ONE hipGraphLaunch; the returned handle borrows the job's arrays until it is freed (up to 3 live
 * handles per key and stream, further calls take the ordinary path).  Same results, same deferred
 * completion; a result that outgrows the captured capacities is redone exactly as always.
 * SDFK_OPT_GRAPHS = 0 switches this off, 2 applies it to every grid size. */
int sdfk_sample_march(const sdfk_program* p, const float min[3], const float max[3],
                      int32_t nx, int32_t ny, int32_t nz, int32_t clip_to_bounds,
                      float iso_value, int32_t step, sdfk_mesh** out);
/* Captured jobs alive, graph launches so far, device bytes the captured jobs hold. */
int sdfk_graph_stats(int64_t* jobs, int64_t* launches, int64_t* device_bytes);

/* Two-phase form for Z-slab sharding (one process per GPU).  `v` is a slab whose planes
 * cover the cell layers [layer_begin, layer_end) (global layer indices) plus context:
 * two planes below layer_begin (unless that reaches plane 0) and one plane above
 * layer_end (unless that reaches the last plane).  begin: classify + count, returns the
 * numbers of vertices and triangle indices this slab owns.  finish: emit, with
 * `vertex_base` = sum of the vertex counts of all lower slabs (exchanged by the caller,
 * e.g. with an RCCL all-gather), so that indices are global and the concatenation of the
 * slab meshes in rank order equals the single-device mesh. step must be 1. */
int sdfk_march_begin(const sdfk_volume* v, float iso_value, int32_t layer_begin, int32_t layer_end,
                     sdfk_march_job** job, int64_t* n_vertices, int64_t* n_indices);
int sdfk_march_finish(sdfk_march_job* job, int64_t vertex_base, sdfk_mesh** out);
void sdfk_march_job_free(sdfk_march_job* job);

/* One-call slab forms (deferred completion as above): buffers are sized from the previous call with the
 * same slab shape, classification and emit are queued back to back, and the exact two-phase
 * path is taken only when that guess was too small.  `vertex_base` is added to every index;
 * pass 0 to get slab-local indices and rebase after the gather (sdfk_slabs_rebase). */
int sdfk_march_slab(const sdfk_volume* v, float iso_value, int32_t layer_begin, int32_t layer_end,
                    int64_t vertex_base, sdfk_mesh** out);
int sdfk_sample_march_slab(const sdfk_program* p, sdfk_volume* slab, int32_t clip_to_bounds, float iso_value,
                           int32_t layer_begin, int32_t layer_end, int64_t vertex_base, sdfk_mesh** out);

/* Self-describing slab payload for a single padded all-gather: 64-byte header
 * { int64 n_vertices; int64 n_indices; float min[3]; float max[3]; int32 vertex_bytes; int32 cap_v; int32 idx_bits; int32 flags; pad }
 * followed by Vertices | Colors | Normals (3 floats per vertex each) | Triangles (int32).
 * vertex_bytes = 36, or 24 when the volume had no colours: Colors (all zero) is then left out.
 * cap_v = vertex slots each section is laid out for (sections at 64, 64 + 12 cap_v, ...; indices at
 * 64 + vertex_bytes * cap_v); 0 = dense (cap_v = n_vertices), what sdfk_mesh_pack writes.  Written device
 * to device into `dst` (capacity_bytes); *needed_bytes = header + arrays.  If it does not fit,
 * only the header is written and SDFK_OK is still returned (the caller sees needed > capacity).
 * For a mesh whose job is still queued (deferred completion) nothing waits: the device packs
 * from the job's own counters, *needed_bytes = -1, and the header says what happened -- counts
 * >= 0 (arrays present if they fit the capacity), or nv = ni = -1 when the speculative buffers
 * of that job were too small (complete the mesh with any accessor and pack again). */
#define SDFK_SLAB_HEADER_BYTES 64
int sdfk_mesh_pack(const sdfk_mesh* m, void* dst, int64_t capacity_bytes, int64_t* needed_bytes);
/* One sharded step of a rank in ONE call (what a pipelined driver queues per step; no host wait):
 * [sdfk_lane_begin(lane, wait_hip_event) if lane > 0] sample the slab -> mesh it [sdfk_lane_end(1)].  From the
 * second call for a slab shape on, the mesh is EMITTED STRAIGHT INTO the payload at dst: its arrays are the
 * payload's sections, laid out for the capacities guessed from the previous mesh (cap_v in the header), and the
 * last kernel writes the header -- no pack launch, no second copy.  (The first call, and hints that do not fit
 * capacity_bytes, mesh into buffers of the library and pack.)  The payload header tells the counts (-1: a
 * speculative capacity was too small, redo the step on the exact path). */
int sdfk_slab_enqueue(const sdfk_program* p, sdfk_volume* slab, int32_t clip_to_bounds, float iso_value,
                      int32_t layer_begin, int32_t layer_end, void* dst, int64_t capacity_bytes,
                      int32_t lane, void* wait_hip_event);
/* `gathered` = world payloads of stride_bytes each (device memory, as produced by an
 * all-gather of sdfk_mesh_pack buffers with slab-local indices): adds to the indices of slab r
 * the vertex counts of slabs 0..r-1, in one launch, reading the counts from the headers. */
int sdfk_slabs_rebase(void* gathered, int32_t world, int64_t stride_bytes);
/* Same, and the `world` 64-byte headers are also written to `headers_mirror`: device-accessible
 * (pinned, mapped) HOST memory, so that the host can read the counts after waiting for one event
 * on the stream, without a copy of its own. */
int sdfk_slabs_rebase_mirror(void* gathered, int32_t world, int64_t stride_bytes, void* headers_mirror);

/* ---- Z-slab sharding over the GPUs of one node (SdfEx.ToMesh, Sdf.cs:59-63, one process per GPU) -------------
 * The reference has no distributed path; this is the multi-GPU form of the same call.  The grid is cut into Z slabs
 * of cell layers (rank r owns a contiguous range of the serial z sweep, MarchingCubes.cs:53-82, so the global vertex /
 * triangle order is the concatenation of the slabs in rank order); every rank samples its planes + a 2-plane context
 * (sampling is a pure function of the voxel index, Voxels.cs:99-108: no halo is exchanged), meshes its layers with
 * slab-local vertex ids straight into its section of a gather buffer, and ONE exchange per step moves the slab meshes:
 * the library calls RCCL itself (librccl.so.1, loaded on first use) on a stream of its own -- ncclAllGather, or the
 * same bytes as grouped ncclSend / ncclRecv over every xGMI link at once (SDFK_OPT_DIST_EXCHANGE) -- then one kernel
 * rebases the gathered indices and mirrors the `world` payload headers to the host.
 *
 *   rank 0:  sdfk_dist_unique_id(id)  -> the host hands `id` (128 bytes) to every rank (its own launcher / MPI / a file)
 *   all:     sdfk_init(local_device); sdfk_dist_init(world, rank, id)
 *   one-off: sdfk_dist_to_mesh(...)   -> the whole mesh on every rank, an ordinary sdfk_mesh handle
 *   repeat:  sdfk_dist_session_create(...); { sdfk_dist_submit(s) ... sdfk_dist_collect(s, ...) } with up to `depth`
 *            steps in flight; sdfk_dist_mesh(s, &m) = the mesh of the step collected last
 *
 * Every call below except unique_id / info / slab is COLLECTIVE: all ranks make the same calls in the same order.
 * Decisions that must agree (payload stride, "a rank's speculative buffers were too small: redo this step exactly")
 * are taken from the gathered headers, which every rank sees (csrc/slab_protocol.h). */
#define SDFK_DIST_ID_BYTES 128
int sdfk_dist_unique_id(void* id_out /* SDFK_DIST_ID_BYTES */);
int sdfk_dist_init(int32_t world, int32_t rank, const void* id /* SDFK_DIST_ID_BYTES */);
/* The same with the exchange done by the HOST (ranks that share one GPU, hosts with a transport of their own, tests):
 * `allgather(ctx, send, recv, bytes_per_rank)` gathers `bytes_per_rank` bytes of every rank's HOST buffer `send` into
 * `recv` (world x bytes_per_rank, rank order) and returns 0; blocking.  The library stages the payloads through
 * pinned memory around it; everything else is the same code. */
typedef int (*sdfk_allgather_fn)(void* ctx, const void* send, void* recv, int64_t bytes_per_rank);
int sdfk_dist_init_host(int32_t world, int32_t rank, sdfk_allgather_fn allgather, void* ctx);
/* backend: 0 = not initialised, 1 = RCCL, 2 = host transport */
int sdfk_dist_info(int32_t* world, int32_t* rank, int32_t* backend);
void sdfk_dist_shutdown(void);
/* The partition (no device needed): cell layers [layer_begin, layer_end) of rank `rank`, and the voxel planes
 * [z0, z0 + nz_local) its slab volume holds for them (context planes included, widened to a multiple of 4). */
int sdfk_dist_slab(int32_t nz, int32_t world, int32_t rank, int32_t* layer_begin, int32_t* layer_end, int32_t* z0, int32_t* nz_local);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop    /* (an opaque handle: the type itself -- in the library a class with members -- is not exported) */
#endif
typedef struct sdfk_dist_session sdfk_dist_session;
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif
/* depth = steps that may be in flight (slots: own slab volume and gather buffer each), 1..8. */
int sdfk_dist_session_create(const sdfk_program* p, const float min[3], const float max[3], int32_t nx, int32_t ny, int32_t nz,
                             int32_t clip_to_bounds, float iso_value, int32_t depth, sdfk_dist_session** out);
/* Queue one step (no host wait from the second step on).  SDFK_ERR_INVALID when `depth` steps are in flight. */
int sdfk_dist_submit(sdfk_dist_session* s);
/* Wait for the OLDEST queued step: this rank's slab counts; a step some rank could not fit is redone here by all. */
int sdfk_dist_collect(sdfk_dist_session* s, int64_t* n_vertices_mine, int64_t* n_indices_mine);
/* Per-rank (vertices, indices) of the step collected last: counts[2 * world]. */
int sdfk_dist_counts(const sdfk_dist_session* s, int64_t* counts);
/* The whole mesh of the step collected last (valid call until the next submit reuses that slot): the slab sections of the
 * gather buffer concatenated into an ordinary device-resident mesh -- identical to the single-GPU sdfk_sample_march.
 * (Exchange mode 3: the payloads of that step are exchanged HERE, so the call is collective -- every rank makes it.) */
int sdfk_dist_mesh(sdfk_dist_session* s, sdfk_mesh** out);
/* This rank's OWN slab of the step collected last as a mesh of its own (indices global: + the vertex counts of the slabs before it).
 * Not collective, no payload exchange: with SDFK_OPT_DIST_EXCHANGE = 3 a host assembles the whole mesh from the ranks' slabs, each
 * copied over its own PCIe link to the offsets sdfk_dist_counts gives (vertices: sum of nv of the ranks before; likewise indices). */
int sdfk_dist_slab_mesh(sdfk_dist_session* s, sdfk_mesh** out);
/* The raw gather buffer of the step collected last: world payloads of stride_bytes each (header + sections, indices
 * rebased), device memory owned by the session.  SDFK_ERR_UNSUPPORTED on a rank that received the headers only (exchange mode 3;
 * mode 2 on a rank other than 0): the foreign sections would be a fresh header followed by stale bytes. */
int sdfk_dist_gathered(const sdfk_dist_session* s, void** device_ptr, int64_t* stride_bytes);
/* stats[8] = { stride_bytes, steps submitted, steps redone on the exact path, stride regrowths, exchange mode used,
 *              host nanoseconds spent inside sdfk_dist_submit (total), inside sdfk_dist_collect (total),
 *              depth | 0x100 if the payloads are in the 16-bit index form | fall-backs to int32 indices << 16 } */
int sdfk_dist_stats(const sdfk_dist_session* s, int64_t stats[8]);
/* Which exchange and which payload form are faster on this node's fabric is a measurement: runs steps_per_mode pipelined steps
 * with ncclAllGather and with the direct grouped sends, each with plain payloads and with compact ones (16-bit index offsets:
 * fewer bytes per peer, an encode and a decode pass more), takes the slowest rank's time for each -- the same numbers on every
 * rank -- and keeps the fastest configuration for this session (a change of the payload form agrees the stride again).
 * Collective, nothing in flight; ns_per_config[4] (may be NULL): the agreed times, index = mode + 2 * (compact), -1 = the scene
 * does not fit the compact form; all 0 with the host transport, which has one exchange only.  SDFK_ERR_UNSUPPORTED for a session
 * whose exchange mode is 2 or 3: who holds the mesh is that session's contract, not a candidate (the mode is left alone; after any
 * failure the session keeps the mode it had). */
int sdfk_dist_tune(sdfk_dist_session* s, int32_t steps_per_mode, int64_t* ns_per_config);
/* This rank's slab step WITHOUT the exchange, queued like a step (measurement: "kernel-only" time of a sharded step). */
int sdfk_dist_enqueue_only(sdfk_dist_session* s);
void sdfk_dist_session_free(sdfk_dist_session* s);
/* SdfEx.ToMesh (Sdf.cs:59-63) over all ranks, one call: every rank gets the full mesh. */
int sdfk_dist_to_mesh(const sdfk_program* p, const float min[3], const float max[3], int32_t nx, int32_t ny, int32_t nz,
                      int32_t clip_to_bounds, float iso_value, sdfk_mesh** out);

/* ---- one process, several GPUs (SdfEx.ToMesh, Sdf.cs:59-63: a library call of ONE host process) --------------------------------
 * The sharded step above wants one rank per GPU; a managed host is one process.  A NODE gives every listed device a context of its
 * own and a host thread of the library's own that is the rank: the threads join one RCCL communicator per device (ncclCommInitRank
 * on a shared id -- what one process per GPU does) and run the same Z-slab step side by side (sdfk_dist_session_*: same
 * partition, same exchange, same protocol); the caller posts a scene and gets the WHOLE mesh back as an ordinary sdfk_mesh on
 * the first device (its accessors -- counts, copy, bounds, transform, free -- work from the calling thread).
 *   devices / n_devices: the HIP ordinals of the ranks, in rank order; NULL / 0 = every device of the process.  A device listed
 *   more than once makes ranks that share a GPU: they exchange through host memory (RCCL refuses two ranks on one device) --
 *   for bring-up and tests on a one-GPU box.
 * sdfk_node_to_mesh takes the SDF program as its op list (each rank compiles / loads it on its own device; a repeated scene keeps
 * its programs and its session: the second call is one sharded step).  One call at a time per node.  Free every mesh before
 * sdfk_node_close.  The node's contexts are private: a thread's own sdfk_init context on the same device is independent of them. */
typedef struct sdfk_node sdfk_node;
int sdfk_node_open(const int32_t* devices, int32_t n_devices, sdfk_node** out);
/* world = ranks; backend = 1: RCCL between the ranks, 2: the host transport (ranks share a device) */
int sdfk_node_info(const sdfk_node* node, int32_t* world, int32_t* backend);
int sdfk_node_to_mesh(sdfk_node* node, const sdfk_op* ops, int32_t n_ops, const int32_t out_rgbw[4], int32_t writes_color,
                      const float min[3], const float max[3], int32_t nx, int32_t ny, int32_t nz,
                      int32_t clip_to_bounds, float iso_value, sdfk_mesh** out);
/* The mesh on the HOST, in the two phases every managed caller needs (Mesh.cs:10-13: four exact-length arrays): begin runs the
 * sharded step and returns the totals; copy fills the caller's arrays -- every rank copies ITS slab into its slice (indices global)
 * over its own PCIe link, all ranks at once.  The node's steps leave the mesh sharded (SDFK_OPT_DIST_EXCHANGE = 3 semantics: only
 * the 64-byte headers cross xGMI), so nothing is bound by what a rank would have to receive from the others.  colors3 may be NULL
 * (has_colors = 0: every colour is zero); min / max = Mesh.Measure over the slabs (may be NULL). */
int sdfk_node_mesh_begin(sdfk_node* node, const sdfk_op* ops, int32_t n_ops, const int32_t out_rgbw[4], int32_t writes_color,
                         const float min[3], const float max[3], int32_t nx, int32_t ny, int32_t nz, int32_t clip_to_bounds,
                         float iso_value, int64_t* n_vertices, int64_t* n_indices, int32_t* has_colors);
int sdfk_node_mesh_copy(sdfk_node* node, float* vertices3, float* colors3, float* normals3, int32_t* triangles, float min[3], float max[3]);
void sdfk_node_close(sdfk_node* node);

/* ---- SdfEx.Sample (Sdf.cs:22-47) ----------------------------------------------
 * The SDF at `n` arbitrary points (x, y, z triples): rgbw4[4 i .. 4 i + 3] = (colour, distance) of point i, exactly what the
 * delegate writes into the caller's Vector4 buffer -- a program that only assigns .W (Sdfs.Sphere, Sdf.cs:211) leaves X, Y, Z of
 * every element as the caller had them.  batchSize / maxDegreeOfParallelism of the reference have no meaning here.
 * sdfk_eval_points: host arrays, synchronous; sdfk_eval_points_device: caller-owned device buffers, asynchronous on the
 * library stream. */
int sdfk_eval_points(const sdfk_program* p, const float* points3, int64_t n, float* rgbw4);
int sdfk_eval_points_device(const sdfk_program* p, const void* points3_dev, int64_t n, void* rgbw4_dev);

/* ---- RayMarcher (RayMarcher.cs:45-211) ---------------------------------------
 * RenderDepth (depth != NULL) and / or Render (rgb != NULL) of the program's SDF by sphere
 * tracing: one ray per pixel, `depth_iterations` steps, 6 more evaluations for the normal,
 * Lambert shading and the sky colour exactly as RayMarcher.Render (RayMarcher.cs:134-169).
 * camera_position and view_projection_inverse (row-major M11..M44) are what GetCameraRays
 * (RayMarcher.cs:97-112) derives from ViewTransform / field of view / planes with
 * System.Numerics; the shim computes them with the BCL and passes them in.  Images are
 * FloatData.Values / Vec3Data.Values layout: pixel (column i, row j) at j*width + i, 3 floats
 * per pixel for rgb.  sdfk_raymarch fills host arrays (synchronous); sdfk_raymarch_device
 * leaves the images in caller-owned device buffers, asynchronously on the library stream. */
int sdfk_raymarch(const sdfk_program* p, int32_t width, int32_t height, const float camera_position[3],
                  const float view_projection_inverse[16], float near_plane, float far_plane,
                  int32_t depth_iterations, float* depth, float* rgb);
int sdfk_raymarch_device(const sdfk_program* p, int32_t width, int32_t height, const float camera_position[3],
                         const float view_projection_inverse[16], float near_plane, float far_plane,
                         int32_t depth_iterations, void* depth_dev, void* rgb_dev);

/* ---- KdTree (KdTree.cs) / IterativeClosestPoint (IterativeClosestPoint.cs) -----------------------------------------
 * sdfk_points: a static point set on the device (x, y, z triples), searched for the exact nearest point, the k nearest, or all within a radius.  Static points are
 * numbered in insertion order: the points of sdfk_points_create, then each sdfk_points_add batch appended (KdTree(points),
 * KdTree.AddPoints).  The search structure is a uniform grid of sorted cell lists rebuilt on the device by every create / add;
 * its shape is not part of the contract (the reference's Left / Right / SplitValue / IsLeaf have no counterpart).
 *   - Nearest point of query q (KdTree.Search, KdTree.cs:160-197): the static point p of least
 *     d2 = (dx*dx + dy*dy) + dz*dz (dx = q.x - p.x ..., binary32, no FMA), ties to the LOWEST index (the reference returns
 *     whichever its traversal met first); distance = sqrtf(d2).  A point counts only if sqrtf(d2) < FLT_MAX; if none does
 *     (a NaN / infinite query, overflow) index = -1, distance = FLT_MAX and nearest3 = the first static point (nearest = Point).
 *   - Refused with SDFK_ERR_INVALID: an empty initial set (ArgumentException, KdTree.cs:41-45), static points with a NaN or
 *     infinite coordinate, 2^31 static points or more in total.  Duplicate static points are allowed.
 * sdfk_points_search: host arrays, synchronous; any output may be NULL.  sdfk_points_search_device: caller-owned device
 * buffers, asynchronous on the library stream.  A set belongs to the device context it was made in.  Calls run in the calling
 * thread's current context and stream, like sdfk_eval_points_device.
 * sdfk_points_stats (diagnostics): stats[0..2] = grid cells along x, y, z; stats[3] = candidates (static points whose
 * distance was computed) of the last search made while sdfk_profile_enable(1) was on, stats[4] = its query count. */
typedef struct sdfk_points sdfk_points;
int sdfk_points_create(const float* points3, int64_t n, sdfk_points** out);
int sdfk_points_create_device(const void* points3_dev, int64_t n, sdfk_points** out);
int sdfk_points_add(sdfk_points* s, const float* points3, int64_t n);              /* AddPoints / AddStaticPoints */
int sdfk_points_add_device(sdfk_points* s, const void* points3_dev, int64_t n);
int sdfk_points_count(const sdfk_points* s, int64_t* n);                           /* TotalPoints */
int sdfk_points_search(const sdfk_points* s, const float* queries3, int64_t n, int32_t* index, float* distance, float* nearest3);
int sdfk_points_search_device(const sdfk_points* s, const void* queries3_dev, int64_t n, void* index_dev, void* distance_dev,
                              void* nearest3_dev);
int sdfk_points_stats(const sdfk_points* s, int64_t stats[5]);
void sdfk_points_free(sdfk_points* s);
/* k nearest / within a radius (extensions: the reference's KdTree has neither).
 * Order: static points are ordered by the pair (d2, index): d2 = (dx*dx + dy*dy) + dz*dz in binary32 without FMA (the formula of
 * sdfk_points_search), index = the insertion index; the smaller d2 first, equal d2 to the LOWER index.  A point counts only under
 * the rule above (sqrtf(d2) < FLT_MAX): for a NaN or infinite query, or on overflow, no point counts.  distance = sqrtf(d2),
 * correctly rounded.
 * Within a radius: a counting point is within r iff sqrtf(d2) <= r -- decided on the f32 distance, so a point at distance exactly r
 * is within r and not within nextafterf(r, 0).  r = +inf: every counting point.  r < 0 or NaN: SDFK_ERR_INVALID.
 *   - sdfk_points_knn: row i of index / distance (n rows of k) holds the first min(k, counting points within max_distance) points
 *     of that order, ascending; the remaining slots hold index = -1 and distance = FLT_MAX; found[i] = the number of real entries.
 *     Any output may be NULL.  1 <= k <= 64, anything else is SDFK_ERR_INVALID (larger neighbourhoods: the radius query);
 *     max_distance follows the radius rules (+inf: no limit).  With k = 1 and max_distance = +inf, index and distance equal
 *     sdfk_points_search's bit for bit.
 *   - sdfk_points_radius_count, then sdfk_points_radius_fill (the caller owns the result arrays, so their size comes first):
 *     count writes offsets[0..n], the exclusive prefix sums of the neighbours per query, offsets[n] = the total.  fill writes query
 *     i's neighbours to index / distance [offsets[i], offsets[i+1]), ascending in the same order (distance may be NULL): a query's
 *     segment cut to k is its sdfk_points_knn row with max_distance = radius.  fill with offsets that are not count's for the same
 *     set, queries and radius is undefined: the host form refuses offsets that do not start at 0 or do not ascend
 *     (SDFK_ERR_INVALID) and otherwise leaves unspecified contents; the _device form trusts them, and offsets that reach beyond the
 *     caller's arrays make it write outside them.
 * The plain forms take host arrays and are synchronous.  The _device forms take caller-owned device buffers and are asynchronous
 * on the library stream (the caller reads offsets[n] itself, after a synchronise).  While sdfk_profile_enable(1) is on,
 * sdfk_points_stats[3..4] report the candidates and queries of the last knn / radius_count / radius_fill call as well (such a
 * call synchronises). */
int sdfk_points_knn(const sdfk_points* s, const float* queries3, int64_t n, int32_t k, float max_distance,
                    int32_t* index /* n*k */, float* distance /* n*k */, int32_t* found /* n */);
int sdfk_points_knn_device(const sdfk_points* s, const void* queries3_dev, int64_t n, int32_t k, float max_distance,
                           void* index_dev, void* distance_dev, void* found_dev);
int sdfk_points_radius_count(const sdfk_points* s, const float* queries3, int64_t n, float radius, int64_t* offsets /* n+1 */);
int sdfk_points_radius_count_device(const sdfk_points* s, const void* queries3_dev, int64_t n, float radius, void* offsets_dev);
int sdfk_points_radius_fill(const sdfk_points* s, const float* queries3, int64_t n, float radius, const int64_t* offsets,
                            int32_t* index /* total */, float* distance /* total; may be NULL */);
int sdfk_points_radius_fill_device(const sdfk_points* s, const void* queries3_dev, int64_t n, float radius, const void* offsets_dev,
                                   void* index_dev, void* distance_dev);
/* ---- Point clouds: normals and volumes (extensions: the reference stops at IterativeClosestPoint) ---------------------------------
 * The static points of a set as a surface: a normal per point from its neighbourhood, and the set with normals as a signed
 * distance volume -- scan -> sdfk_icp_register -> sdfk_points_normals -> sdfk_points_to_volume (with a band) -> sdfk_volume_redistance
 * -> programs, meshes.  Both are ONE function of their inputs, computed by csrc/points_normals.h (binary64 from the f32 inputs,
 * + - * / and sqrt only, each correctly rounded, in the order given, no contraction, one rounding to f32 per result), restated in
 * tests/pointcloud_model.py and compared bit for bit.  Neighbours are sdfk_points_knn's: the same (d2, index) order, d2 formula
 * and max_distance rule; m = the number found.
 *
 * sdfk_points_normals: for every static point i (insertion order), 3 <= k <= 64:
 * 1. Neighbours: the sdfk_points_knn row of p_i (k, max_distance) -- the point itself and any duplicates included.
 * 2. Covariance: q_j = p_j - p_i per component; mean = (the sum of the q_j in neighbour order) / m; with d = q_j - mean the six
 *    sums c00 += d0 d0, c01 += d0 d1, c02 += d0 d2, c11 += d1 d1, c12 += d1 d2, c22 += d2 d2 in neighbour order (not divided by
 *    m: nothing below depends on the scale).
 * 3. Eigenvectors: cyclic Jacobi on the symmetric 3x3, V = I at first; exactly 8 sweeps, each over the pairs (p, q) = (0,1), (0,2),
 *    (1,2), r the third index.  A pair whose a_pq is exactly 0 is skipped.  Otherwise theta = (a_qq - a_pp) / (2 a_pq);
 *    t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0; c = 1 / sqrt(t t + 1); s = t c; a_pp -= t a_pq;
 *    a_qq += t a_pq; a_pq = 0; (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq); every row of V: (v_kp, v_kq) = (c v_kp - s v_kq,
 *    s v_kp + c v_kq).  The eigenvalues l are the diagonal.  n = the column of V of the least l (ties: the lowest column), divided
 *    by its length sqrt((n0 n0 + n1 n1) + n2 n2).
 * 4. Orientation: with a viewpoint w (n_viewpoints = 1: one for all; = the number of static points: one each; = 0: none),
 *    d = ((w0 - p0) n0 + (w1 - p1) n1) + (w2 - p2) n2; d < 0 flips n.  With no viewpoint, or d exactly 0, the component of n of
 *    largest magnitude is made positive (ties: the lowest axis).  That is NOT a consistent orientation of a closed surface; one
 *    without a viewpoint is sdfk_points_orient_normals' (below), applied to these normals afterwards.
 * 5. normal = n rounded to f32; variation = (float)(max(l_min, 0) / ((l_0 + l_1) + l_2)) (surface variation: 0 on a plane, up to
 *    1/3).  The covariance is positive semi-definite, so an l_min below zero is rounding noise (an exactly planar neighbourhood,
 *    which every three points are, ends there as often as not): it counts as zero and the variation is +0.0, never negative.
 *    Only the numerator is clamped; the denominator is the sum of the diagonal as it stands.
 * 6. Degenerate: m < 3, or (c00 + c11) + c22 == 0: normal = (0, 0, 0), variation = 0.  A collinear neighbourhood gives a
 *    deterministic but meaningless direction.
 * 7. SDFK_ERR_INVALID: k outside [3, 64], a NaN or negative max_distance, n_viewpoints not 0, 1 or the number of static points, a
 *    NaN or infinite viewpoint (host form; the _device form does not read them on the host: such a d is compared as it comes, a
 *    NaN one falling to the rule without viewpoint).  normals3 / variation may be NULL.
 *
 * sdfk_points_to_volume: normals3 holds one normal per static point (sdfk_points_normals' or the caller's; finite, not checked);
 * 1 <= k <= 64; max_distance > 0, +inf allowed (SDFK_ERR_INVALID otherwise, and for a volume without storage).  The value is
 * (x - p) . n: normals point to the positive (outside) side.  Every voxel of `v` (a whole volume or a slab, rows padded as
 * sdfk_volume_row_pitch says) is evaluated at its cell centre x, the f32 centres sdfk_sample and sdfk_trimesh_to_volume use:
 * 1. Neighbours: the sdfk_points_knn row of x (k, max_distance).  Those whose normal is (0, 0, 0) are skipped; if none is left (or
 *    none was found) the voxel is UNKNOWN.
 * 2. Cut-off: h2 = the d2 of neighbour k - 1 when m == k, else the greatest d2 within max_distance (FLT_MAX for +inf).
 * 3. Blend over the unskipped neighbours in order: e_j = ((x0 - p0) n0 + (x1 - p1) n1) + (x2 - p2) n2; when h2 > 0: t = d2_j / h2,
 *    u = 1 - t, w = u u, S += w e_j, W += w.  value = S / W when W > 0, else e of the first unskipped neighbour (k = 1: Hoppe's
 *    tangent-plane distance; h2 == 0; every d2 equal).  A neighbour that enters or leaves the set does so with weight 0, so
 *    the field is continuous where the set changes.  The value is rounded to f32, then clamped to [-max_distance, max_distance].
 * 4. Unknown voxels get +-max_distance, the sign carried from the known ones (a known value < 0 is negative, anything else
 *    positive) by three passes: along every line in z an unknown voxel takes the last sign below it, the ones below the first sign
 *    the first sign above; lines still without a sign repeat this along y with what the z pass left, then along x; a volume
 *    without any known voxel becomes +max_distance.  This is right where the band of known voxels covers the surface, so that
 *    every sign change happens inside it (a closed surface, a band of at least a voxel's diagonal, points no sparser than the band);
 *    otherwise -- an open scan, a band thinner than the sampling -- it is deterministic, not meaningful.
 * 5. stats (may be NULL; reading them synchronises): [0] known voxels, [1] unknown voxels, [2] candidates and [3] queries of the
 *    call when sdfk_profile_enable(1) is on (else 0; sdfk_points_stats[3..4] report them too).
 * 6. Colours are left as they are (sdfk_points_to_volume_colors, below, writes them from per-point colours).  Cached sign bits of the volume are dropped, as for a write through sdfk_volume_device_ptrs.
 * The plain forms take host arrays and are synchronous; the _device forms take device arrays and are asynchronous on the library
 * stream (unless stats or profiling make them wait). */
int sdfk_points_normals(const sdfk_points* s, int32_t k, float max_distance, const float* viewpoints3, int64_t n_viewpoints,
                        float* normals3 /* n*3 */, float* variation /* n */);
int sdfk_points_normals_device(const sdfk_points* s, int32_t k, float max_distance, const void* viewpoints3_dev, int64_t n_viewpoints,
                               void* normals3_dev, void* variation_dev);
int sdfk_points_to_volume(const sdfk_points* s, const float* normals3, sdfk_volume* v, int32_t k, float max_distance, int64_t stats[4]);
int sdfk_points_to_volume_device(const sdfk_points* s, const void* normals3_dev, sdfk_volume* v, int32_t k, float max_distance,
                                 int64_t stats[4]);
/* ---- Point clouds: a consistent orientation (extension) ------------------------------------------------------------------------
 * sdfk_points_to_volume wants normals that point outside.  A viewpoint gives that for what one sensor position sees; a merged scan,
 * the vertices of a mesh whose normals were lost, or a cloud of unknown origin has none.  sdfk_points_orient_normals flips the sign
 * of some of the given normals so that neighbouring normals agree and the top of every connected piece points up (Hoppe's seed
 * rule), and changes nothing else: a parallel, deterministic region growing over the k-nearest graph that accepts confident edges
 * first.  It is ONE function of its inputs, computed by csrc/points_orient.h (binary64 from the f32 inputs, no contraction),
 * restated in tests/orient_model.py and compared bit for bit.  Inputs: the static points p_i (insertion order), normals3 (one
 * normal per static point), k, max_distance, max_seeds.
 * 1. Graph: row i is the sdfk_points_knn row of p_i for (k, max_distance): the same order, d2 formula and max_distance rule; the
 *    point itself and any duplicates are included.  2 <= k <= 64.
 * 2. Validity: a normal is VALID iff its three components are finite and not all zero (either sign of zero).  An invalid normal is
 *    never oriented and never a source; it is returned untouched and counted.
 * 3. Dot: dot(i, j) = (n_i0 n_j0 + n_i1 n_j1) + n_i2 n_j2 in binary64 from the f32 inputs as given (the products are exact).  The
 *    weight of the edge is |dot|.
 * 4. State: every point is UNORIENTED, or ORIENTED IN ROUND r with a sign s = +-1.  Rounds are numbered from 1; every seed and
 *    every propagation round takes one number.
 * 5. Seed round: among the unoriented valid points the one of greatest p_z (f32 compare; -0 equals +0, a NaN p_z counts as -inf),
 *    ties to the lowest index.  Its sign makes n_z positive; when n_z == 0 the component of largest magnitude is made positive,
 *    ties to the lowest axis (sdfk_points_normals' step 4).  The level is set to 0.
 * 6. Propagation round r at level L, thresholds T = {0.9375, 0.75, 0.5, 0.0}: every unoriented valid point i looks at the entries
 *    j of its row that are valid and were oriented in a round < r, and among them takes the one of greatest |dot(i, j)|, ties to
 *    the first in row order.  If that weight is >= T[L], i becomes oriented in round r with s_i = -1 if dot(i, j) * s_j < 0, else
 *    +1.  Every point decides from the state at the end of round r - 1 (Jacobi), so the result does not depend on scheduling.  If
 *    the round oriented nothing, L becomes L + 1, otherwise L stays; past the last level the growth of this seed is over.  The
 *    level never goes back up within a seed; every new seed starts at level 0.
 * 7. Steps 5 and 6 repeat while unoriented valid points remain and fewer than max_seeds seeds were used (max_seeds >= 1).  What
 *    then remains is UNREACHED and returned untouched.
 * 8. Output: n_i with the sign bit of each component flipped where s_i = -1: bit-identical to the input up to sign.  stats (may be
 *    NULL): [0] rounds, seed rounds and the propagation rounds that oriented nothing included; [1] seeds; [2] normals flipped;
 *    [3] unreached; [4] invalid; [5..8] points oriented at each level (the seeds are in none).
 * 9. SDFK_ERR_INVALID: k outside [2, 64], a NaN or negative max_distance, max_seeds < 1, a NULL normals3.  (A set always holds a
 *    point: sdfk_points_create refuses an empty one.)
 * Limits (Hoppe's method's): it trusts that the k nearest of a point lie on the same sheet of the surface -- two sheets closer
 * than the sampling, or an edge sharper than the sampling resolves, can carry a wrong sign across; and a dot of exactly 0 carries
 * no information: the normal is kept as it is.  The rounds are about the diameter of the graph, each one a kernel launch.
 * Temporaries of a call, freed at its end: n * k int32 (the rows), n int32 (the round stamps), n bytes (the signs).
 * sdfk_points_orient_normals takes a host array, in place, and is synchronous.  sdfk_points_orient_normals_device takes a device
 * array, in place, on the library stream; it waits internally wherever it reads its control block (once per batch of 32 queued
 * rounds and once per seed), so it has returned only after every round ran; the last flip may still be queued when stats is NULL. */
int sdfk_points_orient_normals(const sdfk_points* s, int32_t k, float max_distance, int32_t max_seeds, float* normals3 /* n*3, in place */,
                               int64_t stats[9]);
int sdfk_points_orient_normals_device(const sdfk_points* s, int32_t k, float max_distance, int32_t max_seeds, void* normals3_dev,
                                      int64_t stats[9]);
/* ---- Point clouds: filters (extension) ------------------------------------------------------------------------------------------
 * Merged scans cover a surface several times over at uneven density, and one stray return stretches the search grid, turns a normal
 * and puts a blob into a volume.  Two filters of the static points p_i (insertion order, n of them) of a set; neither changes the
 * set: the caller makes a new one from the result.  Each is ONE function of its inputs, its arithmetic written once for device and
 * host in csrc/points_filter.h (binary64 from the f32 inputs, one rounding per written operation, no contraction), restated in
 * tests/points_filter_model.py and compared bit for bit.
 *
 * sdfk_points_voxel_downsample: one output point per occupied voxel of the lattice of edge `voxel_size` anchored at `origin` (NULL:
 * (0, 0, 0)), the centroid of the voxel's members.
 * 1. Key: the voxel of p_i along axis a is k_a = floor(((double)p_a - (double)o_a) / (double)size), an integer-valued binary64.  It
 *    is monotone in p_a, so the least and greatest voxel of an axis, kmin_a and kmax_a, are those of the set's bounding box.
 *    SDFK_ERR_INVALID, outputs untouched: a NULL set; a size that is not finite or <= 0; a non-finite origin; an axis with
 *    kmax_a - kmin_a >= 2^21.  The packed key is (k_z - kmin_z) << 42 | (k_y - kmin_y) << 21 | (k_x - kmin_x); two points share a
 *    voxel iff their keys are equal.  (-0.0 and +0.0 share a voxel.)
 * 2. Groups: the members of a voxel are taken in ascending insertion index, and the voxels are output in the order of their lowest
 *    member.  A size below the spacing of the cloud therefore returns the input in order.
 * 3. Centroid, per axis, binary64: the members are cut into chunks of 32 consecutive members in ascending index (the last may be
 *    short); a chunk is summed sequentially from +0.0, the f32 coordinates widened first; the chunk sums are added sequentially, in
 *    order, to +0.0; centroid_a = (float)(sum_a / (double)count).  (A voxel of a million points is 31250 serial additions, not a
 *    million: the chunks are summed side by side.  A lone member comes back bit for bit, except that a coordinate -0.0 comes back
 *    as +0.0: +0.0 + -0.0.)
 * 4. Outputs, the caller's, each of capacity n, any NULL: points_out m x 3 f32; counts m x int32, the members of each voxel; group
 *    n x int32, the output index of every input point (the hook for averaging further per-point data; sdfk_points_voxel_downsample_colors, below, does it on the device).  *m (may be NULL) receives the
 *    number of voxels.  Entries from m on are left as they were.
 * The host form is synchronous.  The device form takes device arrays, runs on the library stream and has finished when it returns
 * (it reads m on the way).  Temporaries of a call, freed at its end: 40 n bytes and 24 bytes per chunk.
 *
 * sdfk_points_outliers: the statistical outlier rule -- a point whose mean distance to its neighbours is far above the cloud's.
 * 1. Row: the sdfk_points_knn row of p_i for (k, max_distance), 2 <= k <= 64: the same order, d2 formula and max_distance rule.  Its
 *    first entry has distance 0 -- the point itself or a duplicate of lower index -- and is dropped.  mean_i = (the sum of
 *    (double)distance_j over the rest, in row order, from 0.0) / (found - 1).  found < 2: the point is ISOLATED, mean_i = +inf; it
 *    takes no part in the statistics and is never kept.
 * 2. Statistics over the c points that are not isolated, binary64, summed in the order of sdfk_icp_register's step 1 (strides of
 *    65536, the halving trees; a point that takes no part adds nothing): mu = sum(mean_i) / c; sigma = sqrt(sum((mean_i - mu)^2) / c),
 *    the two-pass form; thr = mu + (double)std_ratio * sigma.  A point is KEPT iff it is not isolated and mean_i <= thr.  c = 0:
 *    nothing is kept and mu = sigma = thr = 0.0.
 * 3. Outputs, the caller's, each of capacity n, any NULL: mean_distance n x f32, (float)mean_i; keep n x uint8; index_out the kept
 *    indices, ascending; points_out the kept points, ready for sdfk_points_create[_device].  *n_kept (may be NULL) receives their
 *    number.  stats (may be NULL): [0] kept, [1] removed (not isolated, above thr), [2] isolated, [3..5] the bits of mu, sigma, thr.
 *    Entries of index_out / points_out from n_kept on are left as they were.
 * 4. SDFK_ERR_INVALID, outputs and stats untouched: a NULL set; k outside [2, 64]; a std_ratio that is NaN, negative or infinite
 *    (+inf * sigma is a NaN where sigma = 0, and no mean is <= a NaN); a NaN or negative max_distance.  No accepted argument gives
 *    a NaN in mu, sigma or thr.
 * Host and device forms as above; both have finished when they return.  Temporaries: 12 n bytes. */
int sdfk_points_voxel_downsample(const sdfk_points* s, float voxel_size, const float origin[3], float* points_out /* n*3 */,
                                 int32_t* counts /* n */, int32_t* group /* n */, int64_t* m);
int sdfk_points_voxel_downsample_device(const sdfk_points* s, float voxel_size, const float origin[3] /* host */, void* points_out_dev,
                                        void* counts_dev, void* group_dev, int64_t* m);
int sdfk_points_outliers(const sdfk_points* s, int32_t k, float std_ratio, float max_distance, float* mean_distance /* n */, uint8_t* keep /* n */,
                         int32_t* index_out /* n */, float* points_out /* n*3 */, int64_t* n_kept, int64_t stats[6]);
int sdfk_points_outliers_device(const sdfk_points* s, int32_t k, float std_ratio, float max_distance, void* mean_distance_dev, void* keep_dev,
                                void* index_out_dev, void* points_out_dev, int64_t* n_kept, int64_t stats[6]);
/* ---- Point clouds: colours (extension) ------------------------------------------------------------------------------------------
 * The rest of the library moves colour and distance together (programs write Colors next to Values, sdfk_trimesh_to_volume blends
 * vertex colours, sdfk_volume_redistance copies them, the mesher interpolates them onto vertices); these calls do it for point
 * clouds, so that a coloured scan becomes a coloured mesh without leaving the device, and a mesh made any other way can be
 * re-coloured from a scan.  A "colour" is three f32 per static point, in insertion order (colors3, n x 3).  Nothing is clamped and
 * nothing is checked for finiteness, and nothing is specific to RGB: normals averaged through the same calls are as legitimate.
 * Each call is ONE function of its inputs, its arithmetic written once for device and host in csrc/points_color.h (binary64 from the
 * f32 inputs, + - * / only, one rounding per written operation, no contraction, one rounding to f32 per result), restated in
 * tests/pointcloud_color_model.py and compared bit for bit.
 *
 * sdfk_points_blend_colors: the colour at every query x, 1 <= k <= 64, max_distance by the rule of sdfk_points_knn (+inf allowed):
 * 1. Row: the sdfk_points_knn row of x for (k, max_distance): the same order, d2 and bound; m = the number found.  A point's normal
 *    plays no part (there is none here), so no neighbour is skipped.  A query with a non-finite coordinate finds nothing.
 * 2. m == 0: the colour is (+0, +0, +0) and found = 0.
 * 3. Cut-off: h2 is that of sdfk_points_to_volume's step 2: the d2 of neighbour k - 1 when m == k, else the greatest d2 within
 *    max_distance (FLT_MAX for +inf).
 * 4. When h2 > 0, over the neighbours in row order: t = (double)d2_j / (double)h2, u = 1 - t, w = u u, W += w, and per channel c
 *    S_c += w * (double)c_jc -- three separate sums, each from +0.0.
 * 5. W > 0: out_c = (float)(S_c / W).  Otherwise (h2 == 0; k == 1; every d2 equal to h2): out_c is the first neighbour's channel, bit
 *    for bit -- so k = 1 is nearest-point colouring.  As with the distances, a neighbour enters or leaves the set with weight 0.
 * 6. Outputs, each may be NULL: colors_out n x 3 f32, found n x int32.  SDFK_ERR_INVALID: a NULL set, NULL colors3, k outside
 *    [1, 64], a NaN or negative max_distance.
 * The host form is synchronous; the _device form is asynchronous on the library stream, as sdfk_points_knn_device.
 *
 * sdfk_points_to_volume_colors: sdfk_points_to_volume with colors3.  The volume must have colour storage (SDFK_ERR_INVALID
 * otherwise, and for NULL colors3).  Values and stats are bit for bit what sdfk_points_to_volume gives for the same arguments.
 * Colors, in the volume's padded-row layout: at every voxel the function above at the cell centre for the same (k, max_distance) --
 * one walk per voxel, its neighbour list feeding both blends.  A voxel with no point within max_distance gets zero colours (as
 * beyond sdfk_trimesh_to_volume's band); a colour is defined wherever a point was found, also where every neighbour lacks a normal
 * and the value is unknown.  Colours are not filled beyond the band: a mesh vertex gets a sound colour when both voxels of its edge
 * found a point, which is the case under the condition step 4 of sdfk_points_to_volume states (a band of at least a voxel's
 * diagonal, points no sparser than the band).  Cached sign bits are dropped, as there.  Host and _device forms as there.
 *
 * sdfk_points_voxel_downsample_colors: sdfk_points_voxel_downsample with colors3 in and colors_out (capacity n x 3; m rows written,
 * may be NULL).  points_out, counts, group and *m are bit for bit those of sdfk_points_voxel_downsample (one sort serves both).
 * colors_out, per channel: the members' mean by exactly the rule of the centroid (filters, step 3): chunks of 32 members in
 * ascending index, each summed sequentially from +0.0; the chunk sums added in order; (float)(sum / (double)count).  (A lone
 * member's channel -0.0 comes back as +0.0, as a coordinate does.)  SDFK_ERR_INVALID as there, and for NULL colors3.  Host and
 * device forms as there; temporaries: those of sdfk_points_voxel_downsample and 24 more bytes per chunk.
 * sdfk_points_outliers needs no such form: it returns the kept indices, and the kept colours are colors3[index_out[i]]. */
int sdfk_points_blend_colors(const sdfk_points* s, const float* colors3 /* n*3 */, const float* queries3, int64_t n_queries, int32_t k,
                             float max_distance, float* colors_out /* n_queries*3 */, int32_t* found /* n_queries */);
int sdfk_points_blend_colors_device(const sdfk_points* s, const void* colors3_dev, const void* queries3_dev, int64_t n_queries, int32_t k,
                                    float max_distance, void* colors_out_dev, void* found_dev);
int sdfk_points_to_volume_colors(const sdfk_points* s, const float* normals3, const float* colors3, sdfk_volume* v, int32_t k,
                                 float max_distance, int64_t stats[4]);
int sdfk_points_to_volume_colors_device(const sdfk_points* s, const void* normals3_dev, const void* colors3_dev, sdfk_volume* v, int32_t k,
                                        float max_distance, int64_t stats[4]);
int sdfk_points_voxel_downsample_colors(const sdfk_points* s, float voxel_size, const float origin[3], const float* colors3 /* n*3 */,
                                        float* points_out /* n*3 */, int32_t* counts /* n */, int32_t* group /* n */,
                                        float* colors_out /* n*3 */, int64_t* m);
int sdfk_points_voxel_downsample_colors_device(const sdfk_points* s, float voxel_size, const float origin[3] /* host */,
                                               const void* colors3_dev, void* points_out_dev, void* counts_dev, void* group_dev,
                                               void* colors_out_dev, int64_t* m);
/* ---- Point clouds: clusters (extension) -----------------------------------------------------------------------------------------
 * "Which points belong together": density clustering of the static points p_i (insertion order, n of them) of a set -- DBSCAN, with
 * Euclidean cluster extraction as its min_points = 1 case.  sdfk_points_outliers removes lone strays; a floating clump of returns
 * (a hand, a tripod, a second object) has small neighbour distances and survives it: sdfk_points_cluster finds it and
 * sdfk_points_select removes it, or splits a scene into objects, before normals, volumes and registration.  Neither changes the
 * set: the caller makes a new one from the result.  The result is ONE function of the inputs with integer outputs only, its
 * decisions written once for device and host in csrc/points_cluster.h, restated in tests/points_cluster_model.py and compared as
 * bits, whatever order the atomics of the label rounds land in.
 *
 * within(i, j) holds iff j is in the sdfk_points_radius_* result of the query p_i for `radius`: the same d2 formula, the same
 * "counts" rule (sqrtf(d2) < FLT_MAX) and the same predicate sqrtf(d2) <= radius on the f32 distance.  d2 is symmetric bit for bit
 * ((a - b)^2 == (b - a)^2 in binary32), so within is symmetric; within(i, i) holds for every point with finite coordinates.
 * 1. Count: count_i = the number of j with within(i, j), the point itself and its duplicates included; an int32 that saturates at
 *    INT32_MAX (unreachable below 2^31 points).
 * 2. Core: core_i iff count_i >= min_points.
 * 3. Clusters: the connected components of the graph on the core points with an edge wherever within holds, numbered 0 .. C - 1 in
 *    ascending order of their lowest core member.
 * 4. Border: a point that is not core and has at least one core point within the radius gets the cluster of the core point that is
 *    first in (d2, index) order: equal d2 goes to the lower INDEX, never to the lower cluster number.  (Classical DBSCAN gives such
 *    a point to whichever cluster reaches it first; this rule depends on no order.)
 * 5. Noise: every other point gets the label -1.
 * 6. Sizes: sizes[c] = the members of cluster c, core and border.
 * 7. Reductions: min_points = 1 is Euclidean clustering -- every point (of finite coordinates) is core and nothing is noise;
 *    radius = 0 clusters exact duplicates only; radius = +inf makes every counting point a neighbour.
 * 8. SDFK_ERR_INVALID, outputs and stats untouched: a NULL set; a radius that is NaN or negative; min_points < 1.
 * Outputs, the caller's, any NULL: labels n x int32; sizes, capacity n x int32, C entries written, entries from C on left as they
 * were; core n x uint8; counts n x int32; *n_clusters = C.  stats (may be NULL): [0] clusters, [1] core, [2] border, [3] noise
 * points, [4] hook rounds, [5] shortcut launches that worked -- the last two are diagnostics that may vary from run to run.
 * How: one lane per point on the shell walk of every KdTree query; labels by min-hooking with atomicMin and pointer jumping, every
 * hook round repeating the walk -- no edge list is stored.  Temporaries of a call, freed at its end: 8 n bytes (the parents, the
 * root numbers) and n bytes / 4 n bytes for a core / labels array the caller left NULL.  While sdfk_profile_enable(1) is on,
 * sdfk_points_stats[3..4] report the candidates of all walks of the call and n.
 *
 * sdfk_points_select: the points of the kept clusters.  labels: one int32 per static point -- sdfk_points_cluster's, or any other:
 * a point is KEPT iff 0 <= label < n_clusters and keep[label] != 0 (keep: n_clusters bytes, as sdfk_trimesh_select's; not read for
 * any other label).  index_out: the kept indices, ascending; points_out: the kept points, ready for sdfk_points_create[_device];
 * each of capacity n, either may be NULL, entries from n_kept on left as they were; *n_kept (may be NULL) receives their number.
 * n_clusters = 0 keeps nothing.  SDFK_ERR_INVALID, outputs untouched: a NULL set, NULL labels, n_clusters < 0, NULL keep with
 * n_clusters > 0.  Temporaries: 4 n bytes.
 * Nothing is kept on the handle.  The host forms take host arrays and are synchronous.  The _device forms take caller-owned device
 * buffers (keep_dev too), run on the library stream and have finished when they return (they read C / n_kept on the way). */
int sdfk_points_cluster(const sdfk_points* s, float radius, int32_t min_points, int32_t* labels /* n */, int32_t* sizes /* capacity n */,
                        uint8_t* core /* n */, int32_t* counts /* n */, int64_t* n_clusters, int64_t stats[6]);
int sdfk_points_cluster_device(const sdfk_points* s, float radius, int32_t min_points, void* labels_dev, void* sizes_dev, void* core_dev,
                               void* counts_dev, int64_t* n_clusters, int64_t stats[6]);
int sdfk_points_select(const sdfk_points* s, const int32_t* labels /* n */, const uint8_t* keep /* n_clusters bytes */, int64_t n_clusters,
                       int32_t* index_out /* n */, float* points_out /* n*3 */, int64_t* n_kept);
int sdfk_points_select_device(const sdfk_points* s, const void* labels_dev, const void* keep_dev, int64_t n_clusters, void* index_out_dev,
                              void* points_out_dev, int64_t* n_kept);
/* IterativeClosestPoint.RegisterPoints (IterativeClosestPoint.cs:53-196): rigidly moves the caller's points (in place) onto the
 * static set and returns the total transform (row-major M11..M44, System.Numerics row-vector convention) and the number of
 * iterations run.  Each iteration is the reference's: nearest static point of every point, the piecewise distMax from the
 * distance mean and standard deviation, the points with dist <= distMax, C = sum of centred p q^T,
 * R = V diag(1, 1, sign det(V U^T)) U^T, translation = Transform(pmean, Invert(R)) - qmean, step = Invert(R * CreateTranslation(t)),
 * points = Transform(points, step), total = total * step, until the step moves less than both convergence limits or
 * max_iterations steps were made.  Deviations: the reductions and the 3x3 SVD are in f64 (fixed reduction order, bitwise
 * reproducible); R, pmean and qmean are rounded to f32 and every later step is the reference's f32 Matrix4x4 arithmetic.
 * The result is ONE function of its inputs, computed by csrc/icp_solve.h after the reductions (one rounding per written operation,
 * + - * / and sqrt only, no contraction), restated in tests/points_model.py (register_exact) and compared bit for bit:
 * 1. Reductions (every sum of an iteration: d; (d - mean)^2 with mean = sum / n; count, p, q of the kept points; the nine products
 *    (p_a - pmean_a)(q_b - qmean_b) of the kept points, the f32 coordinates widened first): binary64.  Element i is added to the
 *    accumulator (0.0 at first) of thread i % 256 of block (i / 256) % 256, i.e. in strides of 65536 taken in order of i; a point
 *    that is not kept adds nothing.  Within a block a halving tree: s[t] += s[t + o] for t < o, o = 128, 64, ..., 1.  Then the 256
 *    block partials, each added to a 0.0, through the same tree.
 * 2. The filter: m = (float)mean, sd = (float)sqrt(sqsum / n); distMax = m + 3 sd when m < good, else m + 2 sd when m < 3 good, else
 *    m + sd when m < 6 good, else (m + 0.5) + sd, all binary32 (good = good_correspondence_distance, 3 good and 6 good the f32
 *    products); a point is kept iff dist <= distMax.  pmean = sum p / count, qmean = sum q / count.
 * 3. The solve: W = C scaled by the power of two that brings its largest magnitude into [1, 2) (exact; without it the products
 *    below leave binary64 for |C| beyond 2^+-256; C = 0 or non-finite: as it is), V = I.  One-sided Jacobi on the columns of W: at
 *    most 60 sweeps, each over the pairs (i, j) = (0,1), (0,2), (1,2); al = sum_k W_ki W_ki, be = sum_k W_kj W_kj,
 *    ga = sum_k W_ki W_kj (k ascending, from 0.0).  The pair is skipped when ga == 0 or |ga| <= 1e-15 sqrt(al be); otherwise
 *    zeta = (be - al) / (2 ga); t = (zeta >= 0 ? 1 : -1) / (|zeta| + sqrt(1 + zeta zeta)); c = 1 / sqrt(1 + t t); s = c t; every row of
 *    W and of V: (x_i, x_j) = (c x_i - s x_j, s x_i + c x_j).  A sweep without a rotation ends the loop.  sigma_i = sqrt((W_0i W_0i +
 *    W_1i W_1i) + W_2i W_2i); the columns are ordered by descending sigma with a bubble sort that swaps on `<` only (equal sigma
 *    keep their order); V's columns follow.  sigma_0 == 0 (C = 0): U = V = I.  Otherwise u_0 = w_0 / sigma_0; u_1 = w_1 / sigma_1 when
 *    sigma_1 > 1e-12 sigma_0, else (rank 1) u_1 = (u_0 x e) / |u_0 x e|, e the unit axis on which |u_0| is least (ties: the lowest);
 *    u_2 = u_0 x u_1.  d3 = the sign of det V (cofactors along its first row; 0 stays 0), and
 *    R_ab = (V_a0 U_b0 + V_a1 U_b1) + (d3 V_a2) U_b2.
 * 4. R, pmean and qmean are rounded to f32; translation, step, convergence (dtrans = the f32 length of the step's translation <=
 *    converged_max_translation and (|1 - M11| + |1 - M22|) + |1 - M33| <= converged_max_rotation) and total are the f32 Matrix4x4
 *    arithmetic of System.Numerics' software forms (Invert refuses |det| < 1.1920929e-07 with the all-NaN matrix).
 * Refused with SDFK_ERR_INVALID, points and outputs untouched: an empty dynamic set; by sdfk_icp_register also a dynamic point with a
 * NaN or infinite coordinate.  sdfk_icp_register_device does not read the points on the host and leaves them UNCHECKED: such a
 * point's correspondence is (the first static point, FLT_MAX) under the search rule above, and the arithmetic takes its course (a
 * single such point makes the whole transform NaN; among many it is usually filtered out).
 * sdfk_icp_register: host points, synchronous.  sdfk_icp_register_device: device points; returns when the registration has
 * finished (the host reads the iteration count). */
typedef struct sdfk_icp_params {
    int32_t max_iterations;             /* MaxIterations = 100 */
    float good_correspondence_distance; /* GoodCorrespondenceDistance = 0.01 */
    float converged_max_translation;    /* ConvergedMaximumTranslation = 1e-4 */
    float converged_max_rotation;       /* ConvergedMaximumRotation = 1e-5 */
} sdfk_icp_params;
int sdfk_icp_register(sdfk_points* s, const sdfk_icp_params* prm, float* points3, int64_t n, float total[16], int32_t* iterations);
int sdfk_icp_register_device(sdfk_points* s, const sdfk_icp_params* prm, void* points3_dev, int64_t n, float total[16],
                             int32_t* iterations);
/* IterativeClosestPoint.RegisterPoints, point to plane (an extension: the reference has the point-to-point step only).  The same
 * registration with a second metric: each iteration minimises the squared distances of the kept points to the TANGENT PLANES at
 * their nearest static points, which needs one normal per static point (normals3, in insertion order, from sdfk_points_normals or
 * from the caller; their orientation does not matter: the residual is squared, so a flipped normal changes nothing).  Where the
 * static cloud samples a surface and the dynamic points lie between its samples this converges in a few iterations where the
 * point-to-point step stalls.  prm and its defaults, the search, the filter, the stop rule, `total` and the moved points are those of
 * sdfk_icp_register; so is the result: ONE function of its inputs, computed by csrc/icp_solve.h after the reductions, restated in
 * tests/icp_plane_model.py (register_plane_exact) and compared bit for bit.  One iteration:
 * 1. Search and filter as above (steps 1 and 2 of sdfk_icp_register; the distance statistics run over all n points).  A point is
 *    kept iff dist <= distMax, it has a correspondence (index >= 0: the unchecked device form's non-finite points have none) and
 *    the static normal there is not exactly (0, 0, 0) (either sign of zero) -- sdfk_points_normals' degenerate result.
 * 2. count and pmean over the kept points: f64 sums by reduction rule 1, pmean = sum / count.  (No kept point: 0 / 0, and the NaN
 *    takes its course through T into total and the points.)
 * 3. The normal equations, binary64 from the f32 inputs widened first, one rounding per written operation, no contraction.  Per kept
 *    point, q its static point and n the normal there: d = p - pmean; c = (d1 n2 - d2 n1, d2 n0 - d0 n2, d0 n1 - d1 n0);
 *    J = (c0, c1, c2, n0, n1, n2); r = ((p0 - q0) n0 + (p1 - q1) n1) + (p2 - q2) n2.  The 21 products J_a J_b (a <= b), the 6
 *    products J_a r and r r are each reduced on their own by reduction rule 1: A (symmetric 6x6), b, and the sum of r^2.
 * 4. A x = -b.  Cyclic Jacobi on A, V = I at first: kSweeps6 = 8 sweeps, each over the pairs (p, q), p < q, in the order (0,1),
 *    (0,2), ..., (0,5), (1,2), ..., (4,5).  A pair whose a_pq is exactly 0 is skipped; otherwise theta = (a_qq - a_pp) / (2 a_pq);
 *    t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0; c = 1 / sqrt(t t + 1); s = t c; a_pp' = a_pp - t a_pq;
 *    a_qq' = a_qq + t a_pq; a_pq' = 0; for every other index r, ascending: a_rp' = c a_rp - s a_rq, a_rq' = s a_rp + c a_rq; for
 *    every row k of V: v_kp' = c v_kp - s v_kq, v_kq' = s v_kp + c v_kq.  lambda = the diagonal, lambda_max its largest entry.  When
 *    lambda_max is not a positive finite number, x = 0 and nothing is retained.  Otherwise, for k = 0 .. 5 in order, the eigenpairs
 *    with lambda_k > kPlaneTau lambda_max (kPlaneTau = 1e-12, the product rounded once) are retained: dot = 0.0, dot += v_ak (-b_a)
 *    for a = 0 .. 5; coef = dot / lambda_k; x_a += v_ak coef (x = 0.0 at first).  Directions the kept correspondences do not observe
 *    (a plane leaves two translations and a rotation free, a sphere three rotations) get no step.
 * 5. The step.  w_a = x_a / 2 (a < 3); ww = (w0 w0 + w1 w1) + w2 w2; Cayley's rotation R = ((1 - ww) I + 2 w w^T + 2 [w]x) / (1 + ww),
 *    entry by entry R_aa = ((1 - ww) + 2 (w_a w_a)) / (1 + ww), R_01 = (2 (w0 w1) - 2 w2) / (1 + ww), R_10 = (2 (w0 w1) + 2 w2) / (1 + ww),
 *    R_02 = (2 (w0 w2) + 2 w1) / .., R_20 = (2 (w0 w2) - 2 w1) / .., R_12 = (2 (w1 w2) - 2 w0) / .., R_21 = (2 (w1 w2) + 2 w0) / ..;
 *    T_a = (pmean_a + x_{3+a}) - ((R_a0 pmean_0 + R_a1 pmean_1) + R_a2 pmean_2).  R and T are rounded to f32; step is the row-vector
 *    Matrix4x4 with R^T in its upper 3x3 and T in its fourth row (Transform(p, step) = R p + T).  Convergence on the step,
 *    total = total * step and the move of the points are the f32 arithmetic of sdfk_icp_register, step 4.  Cayley's rotation turns by
 *    2 atan(|x| / 2) where the linearisation says |x|: they differ at third order in the angle, which the next iteration removes.
 * stats (int64[4], may be NULL), of the last iteration run (no iteration: zeros): [0] the kept count; [1] the bits of the f64 sum of
 * r^2 over the kept points before the step; [2] 1 if converged; [3] the number of retained eigenvalues.
 * Refused with SDFK_ERR_INVALID, points and outputs untouched: NULL normals, n == 0, a negative max_iterations; by
 * sdfk_icp_register_plane also a dynamic point or a normal with a NaN or infinite component.  sdfk_icp_register_plane_device reads
 * neither on the host and leaves them UNCHECKED.  normals3 holds one normal per static point of s AT THE TIME OF THE CALL.
 * sdfk_icp_register_plane: host arrays, synchronous.  sdfk_icp_register_plane_device: device arrays; returns when the registration
 * has finished. */
int sdfk_icp_register_plane(sdfk_points* s, const sdfk_icp_params* prm, const float* normals3, float* points3, int64_t n, float total[16],
                            int32_t* iterations, int64_t stats[4]);
int sdfk_icp_register_plane_device(sdfk_points* s, const sdfk_icp_params* prm, const void* normals3_dev, void* points3_dev, int64_t n,
                                   float total[16], int32_t* iterations, int64_t stats[4]);

/* ---- Triangle-mesh distance (Mesh -> Voxels) ------------------------------------------------------------------------------
 * A triangle mesh as a signed distance field.  `triangles` holds n_indices int32 vertex indices, three per triangle; colors3
 * (one RGB per vertex) may be NULL.  The arrays are copied: the caller's are not retained.
 * Refused with SDFK_ERR_INVALID: no triangles, n_indices % 3 != 0, 2^31 triangles or more, n_vertices outside [1, 2^31), an
 * index outside [0, n_vertices), a NaN or infinite vertex coordinate (any vertex, referenced or not), and a mesh whose triangles
 * overlap 2^32 or more cells of the search grid in all (the grid has about one cell per triangle; each triangle is binned into
 * every cell its AABB overlaps, so long diagonal slivers count for many).  The device form reads
 * device arrays (e.g. those of sdfk_mesh_device_ptrs: no host round trip), validates them on the device and reports a refusal
 * from the create call, which synchronises.
 * Unsigned distance: for a query p, the triangle of least d2 wins, ties going to the lowest triangle index.  d2 is the squared
 * distance to the closest point on the triangle, computed in binary64 from the f32 inputs by the region-based routine of
 * csrc/trimesh_sdf.h (closest_on_triangle, no contraction); a triangle whose binary64 area term |ab x ac|^2 is exactly zero, or
 * whose face-region numerators are not all >= 0, is measured as its three edges.  distance = (float)sqrt(d2) (correctly
 * rounded); closest3 = the binary64 closest point rounded to f32.
 * sdfk_trimesh_closest: triangle (-1 for a query with a NaN or infinite coordinate), distance (+inf there), closest3 (NaN there)
 * per query; any output may be NULL; host arrays, synchronous.  _device: caller-owned device buffers, asynchronous on the
 * library stream.
 * sdfk_trimesh_to_volume: every voxel of `v` (a whole volume or a slab, rows padded as sdfk_volume_row_pitch says) gets the
 * signed distance at its cell centre, the same f32 centres sdfk_sample evaluates (Voxels.cs:32-34,81,104-106: first centre
 * min + size / n / 2, then + k size / n; slabs use their global z).  The sign counts crossings along z: a triangle crosses column
 * (x_i, y_j) when the column point, moved by (+eps, +eps^2), lies inside its xy projection -- every edge function's sign exact
 * (binary64 TwoSum expansion of six exact products), zero broken by the perturbation; a triangle whose exact projected area is
 * zero covers no column.  On a closed mesh every sheet of surface along a column is counted exactly once, also where the column
 * passes through a projected edge or vertex.  Each crossing has a binary64 z (trimesh_sdf.h z_cross); voxel (i, j, k) is inside
 * iff the number of crossings with z < (double)z_k is odd, and its value is -d inside, d outside.  Parity needs no consistent
 * orientation and handles nested shells; it is meaningless (but deterministic) for open and self-intersecting meshes.
 * The parity sign is well defined exactly when every undirected edge is used an even number of times, which is what
 * sdfk_trimesh_topology reports as odd == 0 ("watertight", see "Triangle meshes: topology").
 * max_distance (>= 0; +inf: exact everywhere): voxels whose f32 distance exceeds it get +-max_distance with the exact sign (and
 * zero colours); every other voxel equals the +inf run bit for bit, colours included.  Without a band, large volumes far from a
 * fine mesh are slow (every voxel searches until its nearest triangle): give a band when only a shell around the surface is needed.  Colours, when the volume has them: the f32 blend of the nearest
 * triangle's vertex colours with its closest-point weights rounded to f32, (ca wa + cb wb) + cc wc; zero when the mesh has
 * none.  Cached sign bits of the volume are dropped, as for a write through sdfk_volume_device_ptrs.  No float atomics: results
 * are bitwise reproducible.
 * sdfk_trimesh_stats (diagnostics): stats[0..2] = grid cells along x, y, z; stats[3] = triangles; stats[4] = triangle-cell pairs
 * binned; stats[5] = candidates (binary64 closest-point evaluations) of the last query or volume made while
 * sdfk_profile_enable(1) was on, stats[6] = its query count; stats[7] = crossing records of the last sdfk_trimesh_to_volume. */
typedef struct sdfk_trimesh sdfk_trimesh;
int sdfk_trimesh_create(const float* vertices3, int64_t n_vertices, const int32_t* triangles, int64_t n_indices, const float* colors3,
                        sdfk_trimesh** out);
int sdfk_trimesh_create_device(const void* vertices3_dev, int64_t n_vertices, const void* triangles_dev, int64_t n_indices,
                               const void* colors3_dev, sdfk_trimesh** out);
int sdfk_trimesh_closest(const sdfk_trimesh* t, const float* queries3, int64_t n, int32_t* triangle, float* distance, float* closest3);
int sdfk_trimesh_closest_device(const sdfk_trimesh* t, const void* queries3_dev, int64_t n, void* triangle_dev, void* distance_dev,
                                void* closest3_dev);
int sdfk_trimesh_to_volume(const sdfk_trimesh* t, sdfk_volume* v, float max_distance);
int sdfk_trimesh_stats(const sdfk_trimesh* t, int64_t stats[8]);
void sdfk_trimesh_free(sdfk_trimesh* t);

/* ---- Triangle meshes: sampling (Mesh.SamplePoints: Mesh -> points) ------------------------------------------------------------
 * n points on the triangles of a mesh, in proportion to area, each with its face normal, blended colour, triangle index and
 * barycentric weights.  ONE function of (mesh, n, seed, flags), computed by csrc/trimesh_sample.h (no contraction); everything
 * that is accumulated is an integer, so no result depends on a summation order and every output is reproducible bit for bit.
 * Weights: for triangle t with f32 vertices a, b, c widened to binary64: e1 = b - a, e2 = c - a, n = e1 x e2 (each product
 * rounded, then one subtraction), A2 = (n.x n.x + n.y n.y) + n.z n.z; A2max = the largest A2;
 * w_t = (uint64)(sqrt(A2_t / A2max) * 2^32) (one division, one correctly rounded root, an exact scaling, truncation), so
 * w_t <= 2^32 and the total stays below 2^63.  A triangle whose area is below 2^-32 of the largest one gets weight 0 and is never
 * sampled.  W = the exclusive 64-bit integer scan of w, W[nt] = total.  A mesh in which no triangle has an area (A2max == 0) is
 * refused with SDFK_ERR_INVALID ("no triangle has an area"); the handle stays usable for everything else (the topology
 * calls read its weights as zeros).
 * Draws: splitmix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (mod 2^64).
 * Sample s takes h_j = splitmix(seed + (3 s + j + 1) * 0x9E3779B97F4A7C15), j = 0, 1, 2: no state is carried, and without
 * SDFK_TRIMESH_SAMPLE_STRATIFIED sample s does not depend on n.
 * Triangle: flags = 0: r = mulhi64(h0, total).  SDFK_TRIMESH_SAMPLE_STRATIFIED: lo_s = floor(s total / n), computed as
 * (total / n) s + ((total % n) s) / n, and r = lo_s + mulhi64(h0, lo_{s+1} - lo_s): one sample per stratum of the total, so
 * triangle t is drawn n w_t / total times to within less than 2, and the output follows the triangle order.  The triangle is the
 * unique t with W[t] <= r < W[t + 1].
 * Position: k1 = h1 >> 11, k2 = h2 >> 11; if k1 + k2 > 2^53 both are replaced by 2^53 - k; k0 = 2^53 - k1 - k2 (>= 0).  The
 * weights w_i = k_i 2^-53 are exact in binary64 and sum to 1.
 * Outputs per sample (each may be NULL): points3 = (float)((w0 a + w1 b) + w2 c) per axis, in binary64; normals3 =
 * (float)(n_k / sqrt(A2)), the unit face normal of the winding (b - a) x (c - a) -- on the meshes sdfk_march makes this agrees in
 * sign with the vertex normals; colors3 = the f32 blend of sdfk_trimesh_to_volume ((ca wa + cb wb) + cc wc, weights rounded to
 * f32), zeros when the mesh has no colours; triangle = t (int32); weights3 = (float)w0, (float)w1, (float)w2, the weights of that
 * blend, with which a caller blends any other per-vertex attribute to the same bits.
 * stats (may be NULL): stats[0] = triangles of non-zero weight, stats[1] = the total weight.
 * Refused with SDFK_ERR_INVALID: n outside [0, 2^31), unknown flag bits, a mesh without area.  n = 0 returns SDFK_OK and touches
 * nothing.  The weights, A2max and the scan are made once per handle, by its first sampling call, which synchronises to read the
 * total and the refusal; W (8 bytes per triangle plus one) stays on the handle until sdfk_trimesh_free.  After that,
 * sdfk_trimesh_sample_device (caller-owned device buffers) only queues work on the library stream, so sample ->
 * sdfk_points_create_device -> sdfk_icp_register_device never touches the host.  sdfk_trimesh_sample: host arrays, synchronous. */
#define SDFK_TRIMESH_SAMPLE_STRATIFIED 1
int sdfk_trimesh_sample(sdfk_trimesh* t, int64_t n, uint64_t seed, int32_t flags, float* points3, float* normals3, float* colors3,
                        int32_t* triangle, float* weights3, int64_t stats[2]);
int sdfk_trimesh_sample_device(sdfk_trimesh* t, int64_t n, uint64_t seed, int32_t flags, void* points3_dev, void* normals3_dev,
                               void* colors3_dev, void* triangle_dev, void* weights3_dev, int64_t stats[2]);

/* ---- Triangle meshes: topology (Mesh.Components / Topology / SelectComponents: extensions) -------------------------------------
 * The connectivity of the nv vertices and nt triangles (a, b, c) of a handle, as ONE function of the index array, computed by
 * the decisions of csrc/trimesh_topology.h.  Connectivity is BY INDEX ONLY: two vertices with equal positions and different
 * indices are different vertices (welding is not done here).  Every output is an integer and unique given the input: the device
 * gives the same bits whatever order its atomics land in.
 * A triangle with a repeated index (a == b, b == c or a == c) is index-degenerate: it connects nothing, contributes no edges,
 * belongs to no component (label -1) and is counted once in the census.  Two vertices are adjacent iff some triangle that is not
 * index-degenerate holds both; a vertex that no such triangle references has label -1.  The root of a component is its lowest
 * vertex index; components are numbered 0 .. C-1 by ascending root.  vertex_component[v] is that number, triangle_component[t]
 * the number of its first index.
 * Edges: every triangle that is not index-degenerate gives the directed edges (a, b), (b, c), (c, a).  The undirected key of
 * (u, v) is min << 32 | max; the edge is forward iff u < v.  An undirected edge used m times, f of them forward, is a boundary
 * edge iff m == 1, non-manifold iff m >= 3, odd iff m is odd, inconsistent iff m == 2 && f != 1.  It belongs to the component of
 * its vertices.
 * Component row, 8 x int64: triangles, vertices, edges, boundary, non_manifold, odd, inconsistent, area_weight.  area_weight is
 * the sum over the component's triangles of the integer sampling weight w_t of "Triangle meshes: sampling" (area over the largest
 * area, in units of 2^-32); the weights are made if the handle has none yet, and here a mesh in which no triangle has an area
 * gives zeros and is not refused.  There is no floating-point area: that would need a summation order.
 * Census, 8 x int64: components, referenced vertices, distinct edges, boundary, non_manifold, odd, inconsistent, index-degenerate
 * triangles.
 * For the host to derive: Euler characteristic V - E + F; watertight: odd == 0 (exactly the condition under which
 * sdfk_trimesh_to_volume's parity sign is well defined); oriented: inconsistent == 0 && non_manifold == 0.
 * sdfk_trimesh_components: vertex_component (nv) and triangle_component (nt), either may be NULL; *n_components = C; stats[0] =
 * hook rounds run, stats[1] = shortcut launches that worked, stats[2..3] = 0 (n_components and stats may be NULL).  The labels
 * are made once per handle by hook-and-shortcut rounds (min-hooking by atomicMin, pointer jumping one jump per launch; at most
 * nv + 1 hook rounds, else SDFK_ERR_INVALID, which no input reaches) and stay on it (4 bytes per vertex and per triangle) until
 * sdfk_trimesh_free; the call that makes them synchronises, and frees its temporaries (9 nv + 4 bytes) at its end.
 * sdfk_trimesh_topology: census is always complete; component_rows receives the rows of components 0 .. min(C, capacity) - 1,
 * rows beyond `capacity` are not written; either may be NULL.  Temporaries, freed at the call's end: the edge records and their
 * sort (2 x 16 x 3 nt bytes, sorted over only the key bytes nv can set), three uint32 arrays of 3 nt + 1, the rows.
 * sdfk_trimesh_select: keep_component holds C bytes (non-zero: keep).  The kept vertices are exactly the vertices of the kept
 * components, in ascending old index; the kept triangles come in ascending old index with their indices rewritten to the new
 * numbering.  vertex_index_out (capacity nv) / triangle_index_out (nt): the old index of every kept item; triangles_out (3 nt);
 * vertices_out / colors_out (3 nv): gathered, colours zeros when the mesh has none.  Label -1 is never kept, so index-degenerate
 * triangles and unreferenced vertices disappear.  Entries beyond *nv_out / *nt_out are left as they were.  Any output may be
 * NULL.  Keeping nothing gives 0 and 0, which is not an error.
 * The plain forms take host arrays; the _device forms take caller-owned device buffers for the arrays (keep_component_dev
 * included) and host pointers for the counts, census and stats; the outputs of sdfk_trimesh_select_device are ready for
 * sdfk_trimesh_create_device.  The call that makes the labels and every topology and select call synchronise (the counts come
 * back through pointers); sdfk_trimesh_components_device on a handle that has its labels only queues two copies on the library
 * stream.
 * Refused with SDFK_ERR_INVALID, outputs untouched: a NULL handle, a NULL keep_component, a negative capacity, and a handle with
 * 2^32 / 3 triangles or more. */
int sdfk_trimesh_components(sdfk_trimesh* t, int32_t* vertex_component, int32_t* triangle_component, int64_t* n_components, int64_t stats[4]);
int sdfk_trimesh_components_device(sdfk_trimesh* t, void* vertex_component_dev, void* triangle_component_dev, int64_t* n_components,
                                   int64_t stats[4]);
int sdfk_trimesh_topology(sdfk_trimesh* t, int64_t census[8], int64_t* component_rows, int64_t capacity);
int sdfk_trimesh_topology_device(sdfk_trimesh* t, int64_t census[8], void* component_rows_dev, int64_t capacity);
int sdfk_trimesh_select(sdfk_trimesh* t, const uint8_t* keep_component, int32_t* vertex_index_out, int32_t* triangle_index_out,
                        int32_t* triangles_out, float* vertices_out, float* colors_out, int64_t* nv_out, int64_t* nt_out);
int sdfk_trimesh_select_device(sdfk_trimesh* t, const void* keep_component_dev, void* vertex_index_out_dev, void* triangle_index_out_dev,
                               void* triangles_out_dev, void* vertices_out_dev, void* colors_out_dev, int64_t* nv_out, int64_t* nt_out);

/* ---- Triangle meshes: adjacency, smoothing, vertex normals (Mesh.Smooth / RecomputeNormals: extensions) -----------------------
 * Per-vertex gathers over the incidence of a handle's mesh, each ONE function of the input, computed by
 * csrc/trimesh_adjacency.h (binary64 from the f32 inputs, the operations in the order given here, no contraction, one rounding
 * to f32 per value; sqrt and the divisions correctly rounded), restated in tests/mesh_smooth_model.py and compared bit for bit.
 * Incidence is BY INDEX, and index-degenerate triangles (see "Triangle meshes: topology") take no part in it.
 * Neighbours: every triangle (a, b, c) that is not index-degenerate gives the six directed records (a,b), (b,a), (b,c), (c,b),
 * (c,a), (a,c), key = from << 32 | to.  They are sorted (csrc/device_sort.h, over only the key bytes nv can set); nbr_start
 * (nv + 1 x uint32) and nbr (n_entries x uint32) hold the neighbours of every vertex ASCENDING, EACH ONCE: those of v are
 * nbr[nbr_start[v] .. nbr_start[v + 1]).  The number of records with key (v, w) is the number of triangle sides on the undirected
 * edge {v, w}; where it is 1 the edge is a boundary edge and boundary[v] = boundary[w] = 1 (nv bytes, 0 elsewhere).
 * Incident corners (kept on the handle, not handed out): the 3 nt records (vertex, 3 t + k) in (t, k) order, sorted stably by the
 * vertex: the corners of every vertex in ascending (t, k) order.
 * Both are made by the first call that needs them (that call synchronises twice to size the arrays) and stay on the handle until
 * sdfk_trimesh_free: 4 (nv + 1) + 4 n_entries + nv bytes and 4 (nv + 1) + 12 nt bytes.  Temporaries of the making, freed at its
 * end: two record buffers of 16 x 6 nt bytes and two uint32 arrays of 6 nt + 1.  A handle with 6 nt >= 2^32 is refused.
 * sdfk_trimesh_adjacency: *n_entries = the length of nbr (may be NULL); nbr_start, nbr, boundary: each may be NULL -- with all
 * three NULL only the size is returned, so a caller asks twice.  Host arrays, synchronous; _device: caller-owned device buffers,
 * queued on the library stream.
 * sdfk_trimesh_smooth: one STEP with factor s maps positions P to P': a vertex without a neighbour, or a pinned one, keeps its
 * three floats as bits; otherwise per axis acc = (double)P[w0] for the first neighbour, then acc += (double)P[w] over the others
 * in ascending order, mean = acc / (double)degree, P'[v] = (float)((double)P[v] + (double)s * (mean - (double)P[v])).  Steps are
 * Jacobi: each reads the result of the one before.  One ITERATION is a step with lambda, then, if mu != 0, a step with mu
 * (Taubin's lambda | mu: mu < -lambda < 0 does not shrink; mu == 0 is plain Laplacian smoothing).  vertices3_out (nv x 3) = the
 * handle's positions after `iterations` iterations; 0 copies them.  SDFK_TRIMESH_SMOOTH_PIN_BOUNDARY pins the vertices whose
 * boundary byte is set (without it an open mesh shrinks from its rim).  THE HANDLE IS NOT CHANGED: its search grid and packed
 * triangles belong to the old positions; to go on with the smoothed mesh make a new handle (sdfk_trimesh_create_device).  All
 * steps are queued on the library stream without a host wait between them; the host form synchronises once, at the copy out.
 * Temporaries: one or two position arrays.
 * sdfk_trimesh_vertex_normals: positions3 (nv x 3, or NULL: the handle's own) are the positions; triangles are gathered through
 * the handle's indices.  For vertex v: N = the sum (from +0, in ascending (t, k) order of its incident corners, one rounding
 * per add) of the triangle's n = (b - a) x (c - a) as "Triangle meshes: sampling" forms it (area weighting); len =
 * sqrt((N.x N.x + N.y N.y) + N.z N.z); normals3_out[v] = (float)(N_k / len), or with SDFK_TRIMESH_NORMALS_FLIP
 * (float)(-(N_k / len)).  A vertex with no corner, or whose len is 0 or not finite, gets (+0, +0, +0).  On the meshes
 * sdfk_march makes, the unflipped normals point the way its gradient normals do.
 * Refused with SDFK_ERR_INVALID, outputs untouched: a NULL handle, a NULL output, unknown flag bits, a lambda or mu that is not
 * finite, iterations outside [0, 65536], 6 nt >= 2^32. */
#define SDFK_TRIMESH_SMOOTH_PIN_BOUNDARY 1
#define SDFK_TRIMESH_NORMALS_FLIP 1
int sdfk_trimesh_adjacency(sdfk_trimesh* t, uint32_t* nbr_start, uint32_t* nbr, uint8_t* boundary, int64_t* n_entries);
int sdfk_trimesh_adjacency_device(sdfk_trimesh* t, void* nbr_start_dev, void* nbr_dev, void* boundary_dev, int64_t* n_entries);
int sdfk_trimesh_smooth(sdfk_trimesh* t, int32_t iterations, float lambda, float mu, int32_t flags, float* vertices3_out);
int sdfk_trimesh_smooth_device(sdfk_trimesh* t, int32_t iterations, float lambda, float mu, int32_t flags, void* vertices3_out_dev);
int sdfk_trimesh_vertex_normals(sdfk_trimesh* t, const float* positions3, int32_t flags, float* normals3_out);
int sdfk_trimesh_vertex_normals_device(sdfk_trimesh* t, const void* positions3_dev, int32_t flags, void* normals3_out_dev);

/* ---- Triangle meshes: welding (Mesh.Weld: an extension) -------------------------------------------------------------------------
 * The mesh of a handle (nv vertices, nt triangles, optional colours) with the vertices of equal position made one: what a
 * triangle soup (every STL, many OBJ exports), separately meshed pieces put together, or any mesh given as plain arrays needs
 * before the functions above, which work BY INDEX, see its connectivity.  ONE function of the input, `tolerance` and `flags`,
 * computed by the decisions of csrc/trimesh_weld.h, restated in tests/mesh_weld_model.py and compared as bits.  Every decision
 * is made on integers; no position is ever made: nothing is averaged.
 * 1. Group key of a vertex.  tolerance == 0 (exact): the 96 bits of (x, y, z) with -0 mapped to +0 per coordinate -- the handle
 *    holds no NaN and no infinity, so two vertices share a group exactly when their three coordinates are equal as values
 *    (subnormals are their own values).  tolerance > 0 (lattice): the cell (floor(x / tol), floor(y / tol), floor(z / tol)) of a
 *    world-anchored lattice with origin (0, 0, 0), as "Point clouds: filters" forms it (binary64 from the f32 inputs; kmin = the
 *    per-axis least cell over ALL vertices, referenced or not); an axis that spans 2^21 cells or more is refused.  THIS IS A
 *    LATTICE, NOT A BALL QUERY: two vertices closer than `tolerance` on opposite sides of a cell face do not weld, and two
 *    vertices of one cell may be up to sqrt(3) tol apart.
 * 2. Representative.  rep[v] = the lowest vertex index of v's group.
 * 3. Triangles.  Triangle t becomes (rep[a], rep[b], rep[c]) and is KEPT unless that is index-degenerate (see "Triangle meshes:
 *    topology"); with SDFK_WELD_KEEP_DEGENERATE every triangle is kept.
 * 4. Vertices.  v is KEPT iff rep[v] == v and some kept triangle names it; with SDFK_WELD_KEEP_UNREFERENCED every v with
 *    rep[v] == v is kept.  Kept vertices are numbered in ascending old index, kept triangles likewise.  A kept vertex keeps ITS
 *    OWN position and colour bits (the representative's: the lowest index wins).
 * 5. Outputs, any may be NULL; entries beyond the counts are left as they were.  vertex_map (nv): the new index of every old
 *    vertex's representative, -1 where that representative was dropped.  vertex_index_out (capacity nv) / triangle_index_out
 *    (nt): the old index of every new vertex / kept triangle.  triangles_out (3 nt): the rewritten, renumbered indices.
 *    vertices_out / colors_out (3 nv): gathered, colours zeros when the mesh has none.  *nv_out, *nt_out: the counts.
 *    stats[4] = { vertices merged away (nv less the number of groups), triangles dropped as degenerate, representatives dropped
 *    as unreferenced, radix passes run }.
 * 6. What follows.  A mesh with no two equal positions, no index-degenerate triangle and no unreferenced vertex comes back bit
 *    for bit, vertex_map[v] == v.  Welding a welded mesh changes nothing, in both modes (with the same tolerance).  Duplicate
 *    triangles are not removed: the census' non-manifold count shows them.
 * How (csrc/lib_trimesh_weld.hip): one 16-byte record per vertex, sorted stably by key (csrc/device_sort.h) from ascending
 * indices, so that the first record of a group is its lowest index.  Exact mode has 96 key bits for a 64-bit sort key: it sorts
 * by x, rewrites the keys to (z, y) and sorts again.  Only the passes whose byte differs between some two keys are run (the OR of
 * key ^ key[0] over all vertices names them: order-free, and a pass over a byte all keys share moves nothing); lattice mode
 * runs those among the passes its spans can set.  Head flags, a scan, rep; triangle and vertex keep flags, two scans, the gathers.
 * Temporaries, freed at the call's end: two record buffers of 16 nv bytes, 17 nv + 8 bytes of flags and numbers, 4 (nt + 1).
 * THE HANDLE IS NOT CHANGED and keeps nothing of this: the result is another mesh, as after sdfk_trimesh_select.  The plain form
 * takes host arrays; the _device form caller-owned device buffers and host pointers for the counts and stats, and its outputs
 * are ready for sdfk_trimesh_create_device.  Both synchronise (the pass masks, the lattice's box and the counts come back to the
 * host).  Everything welding to nothing (*nt_out == 0) is not an error: it gives 0 and 0 (without
 * SDFK_WELD_KEEP_UNREFERENCED).
 * Refused with SDFK_ERR_INVALID, outputs untouched: a NULL handle, a negative, NaN or infinite tolerance, unknown flag bits, a
 * lattice axis spanning 2^21 cells or more. */
#define SDFK_WELD_KEEP_DEGENERATE 1
#define SDFK_WELD_KEEP_UNREFERENCED 2
int sdfk_trimesh_weld(sdfk_trimesh* t, float tolerance, int32_t flags, int32_t* vertex_map, int32_t* vertex_index_out, int32_t* triangle_index_out,
                      int32_t* triangles_out, float* vertices_out, float* colors_out, int64_t* nv_out, int64_t* nt_out, int64_t stats[4]);
int sdfk_trimesh_weld_device(sdfk_trimesh* t, float tolerance, int32_t flags, void* vertex_map_dev, void* vertex_index_out_dev,
                             void* triangle_index_out_dev, void* triangles_out_dev, void* vertices_out_dev, void* colors_out_dev, int64_t* nv_out,
                             int64_t* nt_out, int64_t stats[4]);

/* ---- Triangle meshes: simplification (Mesh.Simplify: an extension) ---------------------------------------------------------------
 * The mesh of a handle made smaller by VERTEX CLUSTERING (Rossignac & Borrel 1993, with Lindstrom's quadric placement, 2000): the
 * vertices of one cell of a lattice become one vertex, and the triangles that fall on top of each other are cleaned up.  This is
 * welding by lattice with a position MADE instead of one kept; it is not edge collapse.  ONE function of the input, `cellSize`,
 * `placement` and `flags`, computed by csrc/trimesh_simplify.h, restated in tests/mesh_simplify_model.py and compared as bits
 * and integers.  Every decision is made on integers; the arithmetic is binary64 from the f32 inputs, one rounding per written
 * operation in the written order, no contraction, and each output component is rounded to f32 once.
 * 1. Groups.  The group of a vertex is its cell of the world-anchored lattice of size cellSize, exactly the lattice mode of
 *    "Triangle meshes: welding" (the same key, the same refusal of an axis of 2^21 cells or more).  rep[v] = the lowest index of
 *    v's group; groups are numbered by ascending rep; the MEMBERS of a group are its vertices in ascending index.
 * 2. Placement of a group's vertex.
 *    SDFK_SIMPLIFY_REPRESENTATIVE (0): the representative's own position and colour bits; nothing is computed.
 *    SDFK_SIMPLIFY_CENTROID (1): per axis, the members in ascending index are cut into chunks of 32 (the last may be short); a
 *      chunk sum takes its members in order (each widened first), the total takes the chunk sums in order, both from +0.0;
 *      c = total / (double)count, once.  The colour is the same mean of the members' colours (zeros when the mesh has none).
 *    SDFK_SIMPLIFY_QUADRIC (2): with c the centroid above BEFORE its rounding.  For every member in order, for every corner of
 *      its incident-corner list in ascending order (the adjacency of the handle: corners 3 t + k, index-degenerate triangles
 *      listed nowhere), the corner's triangle (p0, p1, p2) in ITS OWN vertex order: q_k = (double)p_k - c per component;
 *      e1 = q1 - q0, e2 = q2 - q0; n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), NOT normalised (the weight of a
 *      triangle is its area squared); d = -((n0 q0x + n1 q0y) + n2 q0z); then the nine sums a00 += n0 n0, a01 += n0 n1,
 *      a02 += n0 n2, a11 += n1 n1, a12 += n1 n2, a22 += n2 n2, b0 += d n0, b1 += d n1, b2 += d n2.  A member's nine sums run
 *      over its corners from +0.0; a chunk's take its members' in order, the total the chunks' in order (the chunking of the
 *      centroid).  A TRIANGLE WITH TWO CORNERS IN THE GROUP COUNTS TWICE, one with three three times: it is reached from each
 *      (a triangle inside the cell has no fixed plane anyway; its weight only pulls toward the planes of its neighbours).
 *      A is decomposed by the cyclic Jacobi of "Point clouds: normals and volumes" (8 fixed sweeps; eigenvalues l_i = the
 *      diagonal, eigenvectors v_i = the columns of V).  l_max = l_0, replaced by l_1 when l_1 > l_max, then by l_2 likewise.
 *      x = (0, 0, 0); for i = 0, 1, 2 in order, when l_i > 1e-3 * l_max:  s = (v_0i (-b0) + v_1i (-b1)) + v_2i (-b2);
 *      t = s / l_i;  x_k = x_k + v_ki t.  No square root of its own and no order enters.  The position is p = c + x.
 *      FALLBACK TO THE CENTROID, counted in stats: when l_max > 0 does not hold, or for some axis a, p_a is not finite or not in
 *      k_a cellSize <= p_a < (k_a + 1) cellSize (binary64; k_a = floor(x_a / cellSize) of the representative, as the lattice
 *      forms it).  A placed vertex therefore never leaves its cell before the final rounding.  Colours as for the centroid.
 * 3. Triangles.  Triangle t becomes (rep[a], rep[b], rep[c]); index-degenerate ones are dropped.  The others are grouped by
 *    VERTEX SET (the sorted triple, whatever the winding).  Default: the lowest triangle index of each set is kept, with its own
 *    winding.  SDFK_SIMPLIFY_KEEP_DUPLICATES: all are kept.  SDFK_SIMPLIFY_CANCEL_PAIRS: a set with an even number of triangles
 *    is dropped entirely, one with an odd number keeps its lowest index -- clustering is a simplicial map, and this rule keeps
 *    the image a cycle mod 2: a mesh whose every edge is used an even number of times (IsWatertight) stays so, which is exactly
 *    when the parity sign of sdfk_trimesh_to_volume is defined.  The two flags together are refused.
 * 4. Vertices.  A group is KEPT iff some kept triangle names it.  Kept groups and kept triangles are numbered in ascending old
 *    (representative / triangle) index.
 * 5. Outputs, any may be NULL; entries beyond the counts are left as they were.  vertex_map (nv): the new number of every old
 *    vertex's group, -1 where the group was dropped.  vertex_index_out (capacity nv): the representative's old index of every
 *    new vertex.  triangle_index_out (nt): the old index of every kept triangle.  triangles_out (3 nt), vertices_out /
 *    colors_out (3 nv).  stats[6] = { vertices merged away (nv less the groups), triangles dropped as degenerate, triangles
 *    dropped as duplicates (cancelled ones included), groups dropped as unreferenced, radix passes run (all sorts), quadric
 *    fallbacks to the centroid (over the KEPT groups: a dropped group is not placed) }.
 * 6. What follows.  Placement 0 with KEEP_DUPLICATES is sdfk_trimesh_weld(t, cellSize, 0) in every output.  Simplifying twice
 *    with one cell size and placement 0 changes nothing the second time.
 * How (csrc/lib_trimesh_simplify.hip): welding's grouping; the group numbers by one scan; per triangle one 16-byte record,
 * sorted stably twice as welding's exact mode sorts 96 bits (by the least group number, then by (greatest above middle)), only
 * through the bytes a group number can set (without KEEP_DUPLICATES: 3 * bytes passes, else none); head flags, a scan, run
 * lengths; keep flags, two scans; one lane per kept group walks group -> members -> corners and places the vertex.
 * THE HANDLE IS NOT CHANGED and keeps nothing of this but the corner lists of its adjacency, which placement 2 makes when the
 * handle has none yet.  The plain form takes host arrays; the _device form caller-owned device buffers and host pointers for
 * the counts and stats, and its outputs are ready for sdfk_trimesh_create_device.  Both synchronise.  A mesh that simplifies to
 * nothing gives 0 and 0 and is not an error.
 * Refused with SDFK_ERR_INVALID, outputs untouched: a NULL handle, a cellSize that is not finite and greater than 0, an unknown
 * placement, unknown flag bits, KEEP_DUPLICATES with CANCEL_PAIRS, a lattice axis spanning 2^21 cells or more, a mesh the
 * adjacency refuses (2^32 / 6 triangles or more). */
#define SDFK_SIMPLIFY_REPRESENTATIVE 0
#define SDFK_SIMPLIFY_CENTROID 1
#define SDFK_SIMPLIFY_QUADRIC 2
#define SDFK_SIMPLIFY_KEEP_DUPLICATES 1
#define SDFK_SIMPLIFY_CANCEL_PAIRS 2
int sdfk_trimesh_simplify(sdfk_trimesh* t, float cellSize, int32_t placement, int32_t flags, int32_t* vertex_map, int32_t* vertex_index_out,
                          int32_t* triangle_index_out, int32_t* triangles_out, float* vertices_out, float* colors_out, int64_t* nv_out,
                          int64_t* nt_out, int64_t stats[6]);
int sdfk_trimesh_simplify_device(sdfk_trimesh* t, float cellSize, int32_t placement, int32_t flags, void* vertex_map_dev,
                                 void* vertex_index_out_dev, void* triangle_index_out_dev, void* triangles_out_dev, void* vertices_out_dev,
                                 void* colors_out_dev, int64_t* nv_out, int64_t* nt_out, int64_t stats[6]);

/* ---- Triangle meshes: ray casting (MeshSdf.RayCast / Occluded / Render, Mesh.ToImage) ----------------------------------------
 * What does this ray hit: the other spatial query of a handle next to the closest triangle.  ONE function of the mesh, the rays and
 * the range, computed by csrc/trimesh_ray.h (no contraction), restated in tests/mesh_ray_model.py as brute force over all triangles
 * and compared bit for bit.  The handle is only read, and nothing about its construction is different.
 *
 * The ray-triangle test is the watertight test of Woop, Benthin and Wald (2013), carried out entirely in binary64 from the f32
 * inputs.  Per ray (origin o, direction d, which need not be a unit vector): kz = the axis of greatest |d|, ties to the lowest
 * axis; kx = (kz + 1) % 3, ky = (kx + 1) % 3, the two swapped when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz],
 * Sz = 1 / d[kz].  Per triangle (a, b, c): A = a - o, B = b - o, C = c - o; Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], likewise
 * Bx, By, Cx, Cy; U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax.  A miss if some of U, V, W is < 0 and some is > 0 (a
 * zero counts as inside); det = (U + V) + W, a miss if det == 0; T = (U (Sz A[kz]) + V (Sz B[kz])) + W (Sz C[kz]); t = T / det.  A
 * hit iff t_min <= t <= t_max and t is finite (compared in binary64; a NaN is a miss).  The two triangles of a shared edge form
 * that edge's function from the same products, so no ray passes between them.
 *
 * The answer for a ray is the hit of least (t, triangle index) over ALL triangles of the mesh: triangle = its index,
 * distance = (float)t in units of |d|, weights3 = (float)(U / det), (float)(V / det), (float)(W / det) -- the weights of a, b, c,
 * in the layout of sdfk_trimesh_sample.  A miss gives triangle = -1, distance = +inf and NaN weights.  A ray with a NaN or
 * infinite origin or direction component, or with a zero direction, is a miss.  Any output may be NULL.
 * flags: SDFK_RAY_ANY_HIT (occlusion queries): triangle = 0 when any triangle is hit within the range and -1 otherwise, the search
 * stops at the first hit it meets, and distance and weights3 must be NULL.  Any other bit is refused.
 * Refused (SDFK_ERR_INVALID, nothing written): a null handle, n < 0 or n >= 2^32, a NaN t_min or t_max, t_min > t_max, an unknown
 * flag, null origins or directions with n > 0.  n == 0 succeeds and touches nothing.
 *
 * How (csrc/lib_trimesh_ray.hip): one lane per ray walks the grid the triangles were binned into, slab by slab along the ray's
 * dominant axis, visiting in each slab the few cells that the ray's box over that slab -- widened by the grid's stated slack --
 * covers, and stops when every unvisited slab begins beyond the best t.  The walk is conservative (csrc/trimesh_ray.h gives the
 * argument), so the answer equals brute force; a host program runs the same walk against brute force without a GPU.  One caveat
 * is stated there: a ray lying in a triangle's plane to within binary64 rounding may be reported by brute force at a t unrelated
 * to the geometry (an exactly coplanar ray has det == 0 and misses).
 *
 * sdfk_trimesh_render: one ray per pixel (i, j) of a width x height image, row-major, generated exactly as sdfk_raymarch's kernel
 * generates it (the same f32 arithmetic, copied op for op into csrc/trimesh_ray.h camera_ray): x = -1 + 2 i / (width - 1),
 * y = 1 - 2 j / (height - 1), v = ((x m[q] + y m[4 + q]) + 0 m[8 + q]) + 1 m[12 + q], v.xyz / v.w - camera, divided by its length.
 * t_min = near_plane, t_max = far_plane (refused like t_min and t_max).  depth[j width + i] = distance (+inf for a miss, which the
 * ray marcher's "depth > far" rule reads as sky); triangle as above; rgb: a miss is the sky (0.5, 0.75, 1.0), a hit is
 * dv c + 0.1 with the ray marcher's constants: the hit point s = camera + r distance (f32, mul then add); the normal is the
 * triangle's binary64 (b - a) x (c - a) divided by its binary64 length ((n0 n0 + n1 n1) + n2 n2 under the root), rounded to f32,
 * negated when (nx rx + ny ry) + nz rz > 0 in f32, the zero vector for a zero cross product; the light vector (5, 5, 10) - s
 * normalised as the ray marcher normalises (v (1 / length) when the length is > 0); dv = max(n . l, 0); c = the f32 blend
 * (ca wa + cb wb) + cc wc of the vertex colours with the f32 weights, or (1, 1, 1) when the mesh has none.  Widths and heights of 1
 * give non-finite rays, as in the ray marcher: those pixels are misses.  Any image may be NULL, but at least one must be given;
 * width, height >= 1 and fewer than 2^31 pixels.
 *
 * The _device forms take device buffers (camera and matrix stay host pointers) and only queue work on the library stream; the
 * plain forms take host arrays and synchronise.  While sdfk_profile_enable(1) is on, a ray cast or render counts as the last
 * query of sdfk_trimesh_stats: stats[5] = the binary64 ray-triangle tests it ran, stats[6] = its rays (that call synchronises).
 * No float atomics: results are bitwise reproducible. */
#define SDFK_RAY_ANY_HIT 1
int sdfk_trimesh_raycast(const sdfk_trimesh* t, const float* origins3, const float* directions3, int64_t n, float t_min, float t_max,
                         int32_t flags, int32_t* triangle, float* distance, float* weights3);
int sdfk_trimesh_raycast_device(const sdfk_trimesh* t, const void* origins3_dev, const void* directions3_dev, int64_t n, float t_min,
                                float t_max, int32_t flags, void* triangle_dev, void* distance_dev, void* weights3_dev);
int sdfk_trimesh_render(const sdfk_trimesh* t, int32_t width, int32_t height, const float camera_position[3],
                        const float view_projection_inverse[16], float near_plane, float far_plane, float* depth, float* rgb,
                        int32_t* triangle);
int sdfk_trimesh_render_device(const sdfk_trimesh* t, int32_t width, int32_t height, const float camera_position[3],
                               const float view_projection_inverse[16], float near_plane, float far_plane, void* depth_dev, void* rgb_dev,
                               void* triangle_dev);

/* ---- Triangle meshes: generalized winding number (MeshSdf.WindingNumber / Contains, Mesh.ToVoxels(sign = "winding")) ---------
 * A sign for meshes that are not watertight.  The winding number of a query q is the sum over the triangles of their signed solid
 * angles seen from q, over 4 pi (Jacobson et al. 2013): on a closed, consistently oriented mesh an integer (0 outside, +1 inside
 * outward-facing triangles, -1 inside inward-facing ones, 2 where two closed pieces overlap, 0 in a cavity whose shell faces the
 * other way), and a smooth function where the mesh is open.  INSIDE means |w| > 1/2, decided on the binary64 sum before it is
 * rounded: the absolute value makes the rule independent of which way the normals point, and an overlap counts as inside (the
 * union; parity gives the XOR).  Far clusters of triangles are replaced by their first-order term (Barill et al. 2018).
 * ONE function of (mesh, query, beta), computed by csrc/trimesh_winding.h (no contraction, no library transcendental), restated
 * in tests/mesh_winding_model.py and compared bit for bit.  All arithmetic is binary64 on the widened f32 inputs, one rounding per
 * written operation; every dot product and squared length is (x0 y0 + x1 y1) + x2 y2.
 *
 * Triangle term.  A = a - q, B = b - q, C = c - q; det = A . (B x C) with B x C = (B1 C2 - B2 C1, B2 C0 - B0 C2, B0 C1 - B1 C0);
 * den = (((|A| |B|) |C| + (A . B) |C|) + (B . C) |A|) + (C . A) |B|; term = atan2(det, den) / (2 pi), which is Omega / (4 pi) of
 * Van Oosterom and Strackee.  atan2 is the routine of csrc/mathops.h kept in binary64 (atan2_64: t = min / max of the absolute
 * values, j = rint(8 t), u = (8 t - j) / (8 + t j), atan(j / 8) from a table + (u + (u u^2) P(u^2)), pi / 2 - . when |y| > |x|,
 * pi - . when x < 0, negated when y < 0; zeros, infinities and NaN as C99 Annex F), never a library's.  Edge cases: q equal to a
 * vertex gives det = +-0, den = +0 and the term +-0.  q in the triangle's plane: outside the triangle the term is det's rounding
 * noise over a positive den, about 0; inside it or on an edge den <= 0 and the term is +1/2 or -1/2 by the sign of det, which
 * there is a zero or rounding noise.  A triangle with two equal vertices has det = +-0 exactly and adds +-0 wherever den > 0,
 * which is everywhere off its segment; on the segment den is zero up to rounding, and the term is +-0 or +-1/2 by that rounding.
 * Three distinct collinear vertices behave like a triangle seen in its plane.  A query with a NaN or infinite
 * coordinate visits nothing: its w is NaN, and it is not inside.
 *
 * Hierarchy (built on the device by the first call that needs it, kept on the handle until sdfk_trimesh_free).  L = the least
 * L >= 0 with 16 * 4^L >= triangles, at most 6.  A lattice of 2^L cells per axis covers the cube whose low corner is the low corner of
 * the mesh's f32 box and whose edge e is the box's greatest extent; a triangle belongs to the cell of its centroid
 * ((a + b) + c) / 3: per axis (int)((centroid - lo) (2^L / e)) clamped to [0, 2^L - 1] (cell 0 when e = 0).  The three cell indices are
 * interleaved (x lowest) into a code; the triangles are sorted by (code, index).  The nodes of level l = 0 .. L are the 8^l
 * prefixes of the codes, the eight children of a node in the order dx + 2 dy + 4 dz; a node's triangles are one run of the sorted
 * order.  Per triangle n = (b - a) x (c - a) and weight = |n|.  The sums of n, of weight * centroid and of weight start from 0 and
 * add, for a cell of level L, its triangles in sorted order, and for a node above, its eight children's sums in child order.
 * N = sum n / 2; P = sum(weight centroid) / sum weight (the centroid of the node's first triangle when that is 0); r2 = the greatest
 * |v - P|^2 over the vertices of the node's triangles.
 *
 * The sum.  w starts at 0 at the root; the walk is depth first, children in child order.  At a node that has triangles, with
 * D = P - q and d2 = |D|^2: if d2 > (beta beta) r2 the node adds (D . N) / (4 pi (d2 sqrt(d2))); otherwise, at level L or with at
 * most 4 triangles, it adds its triangles' terms in sorted order; otherwise its children are visited.  w is added up in exactly this
 * order in binary64 -- one lane owns one query, so no order of lanes or atomics exists to depend on, and no term is rounded on the
 * way.  beta = +inf never takes a cluster term: brute force through the same code.  beta = 0 takes the root's.
 *
 * sdfk_trimesh_winding: per query winding = (float)w and inside = 1 when |w| > 1/2 (w in binary64), else 0; either output may be
 * NULL.  Host arrays, synchronous; _device: device buffers, asynchronous on the library stream once the handle has its hierarchy.
 * Refused (SDFK_ERR_INVALID, nothing written): a null handle, n < 0 or n >= 2^32, beta < 0 or NaN, null queries with n > 0.
 * n == 0 succeeds and touches nothing.
 * sdfk_trimesh_to_volume_signed: sdfk_trimesh_to_volume with the sign chosen.  SDFK_TRIMESH_SIGN_PARITY is sdfk_trimesh_to_volume
 * itself (the same code: beta is ignored).  SDFK_TRIMESH_SIGN_WINDING: distances, colours, the band and slabs are the same; voxel
 * (i, j, k) is negative iff the query at its f32 cell centre is inside as above; no crossing records are made (stats[7] of
 * sdfk_trimesh_stats becomes 0).  On a watertight mesh the two agree wherever no rounding decides (everywhere off the surface).
 * Any other sign_mode, beta < 0 or NaN are refused.  Limits: the cluster term is first order (its error falls as (r / d)^2 per
 * cluster: see DESIGN.md for measured errors per beta); a hole is capped by the |w| = 1/2 level set, not by a minimal surface;
 * values next to such a cap are distances to the mesh's triangles, not to the cap, until sdfk_redistance has run.
 * sdfk_trimesh_winding_stats (diagnostics; never builds anything): stats[0] = L (-1: no hierarchy yet), stats[1] = nodes that
 * have triangles, stats[2] = triangles in the fullest cell of level L, stats[3] = times the hierarchy was built (0 or 1);
 * of the last winding call or winding volume made while sdfk_profile_enable(1) was on (that call synchronises):
 * stats[4] = cluster terms, stats[5] = triangle terms, stats[6] = queries; stats[7] = nodes in all. */
#define SDFK_TRIMESH_SIGN_PARITY 0
#define SDFK_TRIMESH_SIGN_WINDING 1
int sdfk_trimesh_winding(sdfk_trimesh* t, const float* queries3, int64_t n, float beta, float* winding, uint8_t* inside);
int sdfk_trimesh_winding_device(sdfk_trimesh* t, const void* queries3_dev, int64_t n, float beta, void* winding_dev, void* inside_dev);
int sdfk_trimesh_to_volume_signed(sdfk_trimesh* t, sdfk_volume* v, float max_distance, int32_t sign_mode, float beta);
int sdfk_trimesh_winding_stats(const sdfk_trimesh* t, int64_t stats[8]);

/* ---- Redistancing (Voxels.Redistance)---------------------------------------------------------------------------------------
 * dst gets a signed distance to the iso-surface of src, with src's sign at every voxel: a first-order Eikonal solve (Godunov
 * upwind, Jacobi sweeps to the fixed point -- the fast iterative method family, Jeong & Whitaker 2008).  src is not modified
 * (dst may be src: in place).  Colours: copied from src when both volumes have them, zeroed when only dst has.  Cached sign
 * bits of dst are dropped, as for a write through sdfk_volume_device_ptrs.  The result is ONE function of the input, computed
 * by csrc/redistance.h (binary64 from the f32 inputs, the operations in the order given here, no contraction, one rounding to
 * f32 per value; sqrt and the divisions correctly rounded), restated in tests/redistance_model.py and compared bit for bit:
 *   h = (DX, DY, DZ), the f32 cell sizes (max - min) / n widened to binary64; s(x) = (double)v(x) - (double)iso_value;
 *   outside(x) = s(x) > 0.0 -- the strict test marching cubes makes, so src and dst mesh to the same sign pattern.
 * 1. Refusal (SDFK_ERR_INVALID, dst untouched): a NaN or infinite value in src (checked on the device; the call synchronises),
 *    a non-finite iso_value, a NaN or negative max_distance, dst of another shape or box than src, volumes without storage, a
 *    cell size h_a that is not finite or not > 0 (a box with max <= min or a NaN or infinite bound on an axis: sdfk_volume_create
 *    accepts it; the iteration has no fixed point there).  All but the first are decided on the host, before any launch.
 * 2. Front.  x is on the front if one of its six in-range neighbours n has outside(n) != outside(x).  For each axis a with
 *    such a neighbour, t_a = the least (h_a * |s(x)|) / (|s(x)| + |s(n)|) over them (the linear crossing marching cubes places
 *    on that edge).  T0 = 0 if some t_a == 0, else (float)(1 / sqrt(q)), q = the sum of 1 / (t_a * t_a) over the axes that
 *    have a crossing, added in x, y, z order (the distance to the plane through the crossings).  Front voxels are frozen at
 *    T0; every other voxel starts at +inf.
 * 3. Sweep.  T is f32.  One sweep reads T_k only and writes T_k+1 (Jacobi).  For a voxel that is not frozen: per axis
 *    a_i = min(T_k(x - e_i), T_k(x + e_i)) (out of range: +inf), the axes sorted by ascending a_i, ties keeping x, y, z order;
 *    w_i = 1 / (h_i * h_i); u = a_1 + h_1; if u > a_2: A = w_1 + w_2, B = w_1 a_1 + w_2 a_2,
 *    S = (w_1 a_1) a_1 + (w_2 a_2) a_2, D = B B - A (S - 1), u = (B + sqrt(D > 0 ? D : 0)) / A; if that u > a_3: A, B, S each
 *    gain the third axis' term (added last) and u is solved again the same way.  uf = (float)u;
 *    T_k+1(x) = (uf < T_k(x) and uf <= max_distance) ? uf : T_k(x).
 * 4. Fixed point.  Sweeps repeat until one changes nothing (f32 values only ever decrease: it terminates).
 * 5. Result.  m = min(T, max_distance); the value is m where outside, -m elsewhere (v == iso: -0.0, inside, as marching cubes
 *    treats it).  A volume without a front gives +-max_distance everywhere (+-inf unbanded).
 * An upwind value exceeds every a_i it used, so values above max_distance never influence values below it: they are not stored
 * (step 3) and the solve stops expanding there; a banded run equals the clamp of the unbanded one.
 * Schedule (csrc/lib_redistance.hip): tiles of 8^3 voxels; a tile is swept in sweep k + 1 only if it or one of its six face
 * neighbours changed in sweep k -- exactly the full Jacobi sweep, since an update reads the 6-neighbourhood only.  Works on the
 * planes the volume holds (a slab is solved on its own).  Device memory: 8 bytes per voxel of the volume padded to whole tiles.
 * stats (may be NULL; reading them synchronises): [0] sweeps of the full Jacobi iteration, the last one (which changes nothing)
 * included, 0 when there is no front; [1] tile-sweeps executed; [2] front voxels; [3] voxels whose T exceeds max_distance. */
int sdfk_volume_redistance(const sdfk_volume* src, sdfk_volume* dst, float iso_value, float max_distance, int64_t stats[4]);

/* ---- Depth images: fusion and unprojection (DepthFusion, DepthToPoints) ----------------------------------------------------
 * The way from depth frames with poses to a surface (Curless & Levoy 1996): sdfk_volume_integrate_depth averages one frame into
 * a volume of truncated signed distances, sdfk_depth_unproject gives a frame as points.  A depth image is FloatData's layout
 * (pixel (i, j) at j * width + i) and holds the distance ALONG THE PIXEL'S RAY from camera_position: what sdfk_raymarch and
 * sdfk_trimesh_render write.  Both functions are f32 arithmetic on the f32 inputs, every + - * / and sqrt correctly rounded in
 * the order written here, no contraction: csrc/depth_fusion.h, restated in tests/depth_fusion_model.py, compared bit for bit.
 *
 * sdfk_volume_integrate_depth: `values` (D) and `weights` (W) are two volumes of one shape, box and slab (a slab uses its global
 * z); the weights volume needs no colours.  view_projection is the FORWARD matrix ViewTransform x projection, row-major, row
 * vectors (Vector3.Transform): the matrix whose inverse the renders take.  Per voxel, at the f32 cell centre p that sdfk_sample
 * uses (see sdfk_trimesh_to_volume):
 * 1. Project.  c_q = ((p0 m[q] + p1 m[4 + q]) + p2 m[8 + q]) + m[12 + q] for q = 0, 1, 3.  Skipped unless c_3 > 0.
 * 2. Pixel.  u = (c_0 / c_3 + 1) * ((float)(width - 1) * 0.5f), v = (1 - c_1 / c_3) * ((float)(height - 1) * 0.5f): the inverse
 *    of the renders' pixel -> NDC map (pixel 0 at NDC -1).  fu = floorf(u + 0.5f), fv likewise.  Skipped unless 0 <= fu <=
 *    width - 1 and 0 <= fv <= height - 1, compared in float BEFORE any conversion and before the load: a NaN fails every
 *    comparison, and no out-of-range index is ever formed.  i = (int)fu, j = (int)fv.
 * 3. Depth.  d = depth[j * width + i]; r = sqrt((dx dx + dy dy) + dz dz), dx = p0 - cam0 and so on; s = d - r.
 * 4. Classify.  depth_min <= d <= depth_max (false for a NaN) is a SURFACE OBSERVATION: skipped when s < -truncation, else
 *    t = s when s <= truncation, else t = truncation.  With SDFK_FUSE_CARVE_BEYOND a pixel with d > depth_max (+inf included)
 *    says "nothing within range": the voxel is updated with t = truncation when r <= depth_max.  Everything else is skipped.
 * 5. Update.  When W > 0: D' = (W D + weight t) / (W + weight), W' = min(W + weight, max_weight).  Otherwise (a zero, negative
 *    or NaN weight: unseen) D' = t and W' = min(weight, max_weight): whatever D held never enters the arithmetic.
 * 6. Skipped voxels are not written: their bits stay.  Cached sign bits of both volumes are dropped, as for a write through
 *    sdfk_volume_device_ptrs.  Colours are left alone.
 * THE UNSEEN CONVENTION.  An unseen voxel keeps the value it had before its first observation, so the fill of `values` decides
 * what a mesh of the volume shows.  Filled with -truncation and integrated with SDFK_FUSE_CARVE_BEYOND: unseen space is solid,
 * seen-empty space is free (Curless and Levoy's hole filling) -- a fully scanned object meshes watertight, its unscanned
 * interior negative.  Filled with +truncation without carving: the classic open surface, with a spurious sheet one truncation
 * behind every observed surface.  Away from the zero set the values are projective distances (scaled by 1 / cos of the viewing
 * angle, clamped): sdfk_volume_redistance makes them distances again.
 * stats (may be NULL; reading them synchronises): [0] voxels updated; [1] of them, surface observations with s <= truncation;
 * [2] of them, first observations; [3] pixels with depth_min <= d <= depth_max.
 * Refused (SDFK_ERR_INVALID, nothing written): a NULL handle, image, camera, matrix or prm; values == weights; shapes, boxes or
 * slabs that differ, or a volume without storage; width or height < 1, or 2^31 pixels or more; a truncation or weight that is
 * not finite and > 0; max_weight NaN or below weight (+inf allowed); a NaN depth_min or depth_max, or depth_min > depth_max;
 * unknown flag bits.  The host form is synchronous; the _device form (depth_dev a device buffer) queues on the library stream.
 *
 * sdfk_depth_unproject: for every pixel with depth_min <= d <= depth_max, in ascending pixel order: r = the camera ray of the
 * renders (csrc/trimesh_ray.h, camera_ray: view_projection_inverse is the matrix they take), point = cam + r * d, a multiply
 * then an add per component -- for a frame sdfk_trimesh_render made, that render's hit points bit for bit.  colors3 gathers the
 * pixel's rgb (it must be NULL when rgb is NULL), pixel gets j * width + i.  The outputs are compacted (the scan of
 * csrc/device_scan.h) and sized for width * height entries by the caller, who must not rely on what lies beyond *n_valid; any
 * output but n_valid may be NULL.  An image of width or height 1 has non-finite camera rays (the renders leave such frames
 * without a valid depth): a valid depth on such an image yields non-finite points, as camera_ray gives them.  Refused: a NULL
 * depth, camera, matrix or n_valid, colors3 without rgb, and the image and range refusals above.  Reading n_valid synchronises. */
typedef struct sdfk_fusion_params { float truncation, depth_min, depth_max, weight, max_weight; int32_t flags; } sdfk_fusion_params;
#define SDFK_FUSE_CARVE_BEYOND 1
int sdfk_volume_integrate_depth(sdfk_volume* values, sdfk_volume* weights, const float* depth, int32_t width, int32_t height,
                                const float camera_position[3], const float view_projection[16], const sdfk_fusion_params* prm,
                                int64_t stats[4]);
int sdfk_volume_integrate_depth_device(sdfk_volume* values, sdfk_volume* weights, const void* depth_dev, int32_t width, int32_t height,
                                       const float camera_position[3], const float view_projection[16], const sdfk_fusion_params* prm,
                                       int64_t stats[4]);
int sdfk_depth_unproject(const float* depth, const float* rgb, int32_t width, int32_t height, const float camera_position[3],
                         const float view_projection_inverse[16], float depth_min, float depth_max, float* points3, float* colors3,
                         int32_t* pixel, int64_t* n_valid);
int sdfk_depth_unproject_device(const void* depth_dev, const void* rgb_dev, int32_t width, int32_t height, const float camera_position[3],
                                const float view_projection_inverse[16], float depth_min, float depth_max, void* points3_dev,
                                void* colors3_dev, void* pixel_dev, int64_t* n_valid);

/* ---- pinned host arena -------------------------------------------------------
 * Host memory the GPU can write directly (hipHostMalloc), recycled through size-class free lists:
 * destinations inside such a block make sdfk_mesh_copy / sdfk_volume_download / sdfk_raymarch plain
 * DMA transfers at the link rate (512^3 sphere mesh, 33 MB: 0.6 ms).  Into ordinary pageable
 * memory (managed arrays pinned by the shim for the call) the same entry points first touch the
 * destination pages on a small thread pool, which is what a copy into FRESHLY allocated arrays
 * is otherwise dominated by (SDFK_COPY_THREADS in the environment at start-up, SDFK_OPT_COPY_MODE).  The Python mirror allocates
 * Mesh.Vertices/Colors/Normals/Triangles here; a C# shim can do the same for Span<T>/Memory<T>
 * based accessors, while Mesh's public arrays (Mesh.cs:10-13) have to stay managed arrays.
 * sdfk_host_free returns the block to the arena; blocks that are still out at sdfk_shutdown stay valid (they are
 * not reclaimed: sdfk_host_free after a shutdown ignores them). */
int sdfk_host_alloc(int64_t n_bytes, void** out);
void sdfk_host_free(void* p);
/* Makes [p, p + n_bytes) of the caller's pageable memory (freshly allocated managed arrays, pinned for the call) present and
 * writable on the library's thread pool -- what sdfk_mesh_copy does to its destinations anyway, offered separately so that
 * the host can do it WHILE the GPU computes the mesh: sdfk_sample_march (returns at once) -> sdfk_mesh_size_hint ->
 * allocate Vertices / Colors / Normals / Triangles -> sdfk_host_prefault each -> sdfk_mesh_counts (waits) -> sdfk_mesh_copy. */
int sdfk_host_prefault(void* p, int64_t n_bytes);
/* Phases of the last staged device -> pageable-host copy (measurement): stats[5] = { bytes, ns until every chunk was queued,
 * ns until the destination pages were present, ns until done, ns of that spent waiting for the DMA }. */
int sdfk_copy_stats(int64_t stats[5]);
/* What the stream placement found (diagnostics): out[0] = 1 if measured, out[1] = classes found (streams of one class must not be
 * busy together: same hardware queue or same pipe), out[2] = class of lane 0 (the caller's stream), out[3..6] = classes of lanes
 * 1..4 (-1: no placed stream), out[7] = class of the exchange stream of a sharded rank (-1: none kept). */
int sdfk_stream_placement(int32_t out[8]);

/* ---- Mesh (Mesh.cs:8-64) ----------------------------------------------------
 * Vertices/Colors/Normals: 3 floats each per vertex; Triangles: int32 indices
 * (Mesh.cs:10-13).  Vertices/Normals are already transformed to world space
 * (MarchingCubes.cs:85-90, Mesh.cs:47-64). */
int sdfk_mesh_counts(const sdfk_mesh* m, int64_t* n_vertices, int64_t* n_indices);
/* The same WITHOUT waiting: for a mesh whose job is still queued, the counts of the previous mesh of the same grid shape
 * (what its buffers were sized from: exact whenever the scene repeats), *exact = 0; for a finished mesh its counts, *exact = 1.
 * Lets a host allocate (and sdfk_host_prefault) the managed arrays of Mesh.cs:10-13 while the GPU still works. */
int sdfk_mesh_size_hint(const sdfk_mesh* m, int64_t* n_vertices, int64_t* n_indices, int32_t* exact);
int sdfk_mesh_bounds(const sdfk_mesh* m, float min[3], float max[3]);      /* Mesh.Measure */
int sdfk_mesh_copy(const sdfk_mesh* m, float* vertices3, float* colors3, float* normals3,
                   int32_t* triangles);                                      /* any may be NULL */
int sdfk_mesh_device_ptrs(const sdfk_mesh* m, void** vertices3, void** colors3, void** normals3,
                          void** triangles);
/* device-to-device copy into caller-owned device buffers (e.g. torch tensors used as RCCL
 * all-gather inputs), asynchronous on the library stream; any pointer may be NULL */
int sdfk_mesh_copy_device(const sdfk_mesh* m, void* vertices3, void* colors3, void* normals3,
                          void* triangles);
/* Mesh.Transform(Matrix4x4) (Mesh.cs:47-64), in place on the device-resident mesh: positions by Vector3.Transform with
 * `matrix`, normals by Vector3.TransformNormal with `normal_matrix` and Vector3.Normalize, then Mesh.Measure.  Both
 * matrices row-major M11..M44 (row-vector convention of System.Numerics); normal_matrix = Transpose(Invert(matrix with
 * M41 = M42 = M43 = 0, M44 = 1)) exactly as Mesh.cs:49-55 derives it -- BCL calls the shim makes with the BCL itself.
 * Works on every mesh sdfk_march / sdfk_sample_march / sdfk_dist_mesh return, whatever the call history (a handle that borrows a
 * captured job's arrays is transformed in place: the job is busy until the handle is freed); SDFK_ERR_UNSUPPORTED only for the
 * per-rank slab meshes of sdfk_sample_march_slab whose arrays are sections of a gather buffer. */
int sdfk_mesh_transform(sdfk_mesh* m, const float matrix[16], const float normal_matrix[16]);
/* diagnostics: number of active cells, and of case-13 cells with no tiling
 * ("Impossible case 13?", MarchingCubes.cs:365) seen while meshing */
int sdfk_mesh_stats(const sdfk_mesh* m, int64_t* n_active_cells, int64_t* n_case13_cells);
void sdfk_mesh_free(sdfk_mesh* m);

/* ---- measurement hooks (bench.py) ------------------------------------------
 * on = 1: every kernel launch is bracketed by hipEvents on the launch stream (sdfk_profile_get).
 * on = 2: sdfk_sample launches the fused sampling kernel ONLY (no sign-bit transposition, cached
 *         views left invalid), so that the caller can time K back-to-back launches of that one
 *         kernel between two events of its own.  on = 0: normal operation. */
int sdfk_profile_enable(int32_t on);
int sdfk_profile_reset(void);
/* number of distinct kernels recorded; fills name/total milliseconds/launch count */
int sdfk_profile_count(void);
int sdfk_profile_get(int32_t i, const char** name, double* total_ms, int64_t* launches);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SDFKIT_HIP_H */
