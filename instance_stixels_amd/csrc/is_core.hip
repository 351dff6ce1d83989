/*
 * is_core.hip -- C ABI of the gfx950 column-DP core (include/instance_stixels_core.h).
 *
 * Owns what the device half of the reference's Stixels::Initialize / Compute / Finish owns
 * (/root/reference/InstanceStixels/src/Stixels.cu:43-283, 449-637): frame-independent LUTs,
 * per-column scratch (boundary records + object LUT), DP tables, and the launch sequence.
 * There is no CPU fallback: every failure is reported through the return code.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "instance_stixels_core.h"
#include "is_device.h"
#include "is_ground_model.h"
#include "is_launch.h"
#include "is_numerics.h"

#define IS_FLT_HUGE 1e30f
static thread_local char g_err[512] = "";

static int fail_hip(hipError_t e, const char* what, const char* file, int line) {
    snprintf(g_err, sizeof(g_err), "%s returned %s (%d) at %s:%d", what, hipGetErrorString(e),
             (int)e, file, line);
    return IS_EHIP;
}
static int fail_arg(const char* msg) {
    snprintf(g_err, sizeof(g_err), "invalid argument: %s", msg);
    return IS_EINVAL;
}
/* (for the other translation units of the library: is_gather.hip) */
extern "C" int isk_fail(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}
#define HIP_TRY(expr)                                                    \
    do {                                                                 \
        hipError_t e__ = (expr);                                         \
        if (e__ != hipSuccess) return fail_hip(e__, #expr, __FILE__, __LINE__); \
    } while (0)

#define IS_STAGE_SLOTS 4 /* pinned staging ring of the per-frame ground model */

/* The IS_* launch knobs (experiments, A/B runs, tests): environment variables read ONCE in is_ctx_create, never per
 * call; -1 = automatic.  Only plan_call reads them. */
struct Knobs {
    int pw_groups;   /* IS_PW_GROUPS: column groups (streams) of the pairwise DP */
    int p2_split;    /* IS_P2_SPLIT: 1 = k_pw_phase2s, 0 = k_pw_phase2 */
    int p2x;         /* IS_P2X=0: large batches walk phase 2 with k_pw_phase2 (one column per wave) */
    int win_tiles;   /* IS_P1_WIN_TILES: number of DP tiles that stage an fn window at any call size */
    int lut_fused;   /* IS_LUT_FUSED: -1 / 1 = the LUT units run inside the unary DP launch where they can, 0 = never,
                      * 2 = (tests) fused with a WRONG XCC id published: every workgroup distrusts, the repair launches
                      * run, 3 = (tests) the default policy (-1) with the wrong id of 2: the first large call is
                      * repaired, and the context then keeps the table in the prepare launch (DevParams::lutf_repairs) */
    int unary_path;  /* IS_UNARY_PATH, see plan_call */
};

/* Every device block of a context, recorded by alloc(): the context's destroy frees the record, so a buffer added
 * later cannot be left out of it.  (Zero-initialised by the context's calloc.) */
struct OwnedBlocks {
    void* ptr[32];
    int n;
    template <typename T> hipError_t alloc(T** p, size_t bytes) {
        const hipError_t e = n < 32 ? hipMalloc((void**)p, bytes) : hipErrorInvalidValue; /* (full: enlarge ptr) */
        if (e == hipSuccess) ptr[n++] = *p;
        return e;
    }
    void free_all() { while (n > 0) (void)hipFree(ptr[--n]); }
};

struct is_ctx {
    OwnedBlocks owned;       /* every device block below (ALLOC in ctx_init) */
    is_stixel_params params;
    DevParams dp;
    Knobs knobs;
    int device;
    int max_batch;
    int nwaves_unary, nwaves_pairwise;
    /* frame-independent device tables */
    float* d_obj_cost_lut;   /* [D dis][D fn], transposed w.r.t. Stixels.cu:122-129 */
    float* d_obj_cost_fn;    /* [D fn][D dis], as Stixels.cu:122-129: a walk lane's gather stays in one fn row */
    float* d_odr;            /* [D]     object_disparity_range */
    float* d_rcp;            /* [H+1]   RN(1/h) = (float)(1./h), the reference's inverse_height */
    int* d_col_flags;        /* [max_batch*C] 0 = FAST column, see RowRec */
    PruneRec* d_prune;       /* [max_batch*C] branch-and-bound slacks of the column */
    int* d_n_generic;        /* [1] generic-encoding columns of the current call */
    int* d_path_bad;         /* [2] k_unary_path's distrust word of the current call (cleared by the next prepare launch), calls repaired (k_backtrace) */
    int last_unary_path = -1; /* the unary DP of the last unary call: 1 = k_unary_path, 0 = tile path (CallPlan::unary_walk) */
    int last_lut_carry_lds = -1; /* CallPlan::lut_carry_lds of the last call's prepare step (is_debug_lut_carry_lds) */
    /* per-call device inputs */
    /* one block [ground: max_batch x 3 x H floats][instance table: max_batch][vhor: max_batch ints], on
     * the device and in every pinned staging slot: a full batch (the host class's single frame
     * included) travels in ONE copy */
    char* d_stage;
    size_t stage_bytes, stage_off_inst, stage_off_vhor;
    char* h_stage[IS_STAGE_SLOTS];
    float* d_ground;         /* [max_batch][3][H]            (in d_stage) */
    int* d_vhor;             /* [max_batch]                  (in d_stage) */
    /* is_compute_road: the constants of k_ground_model and the table Stixels::FastLog reads (is_ctx_set_ground_model) */
    is_ground_params ground_params;
    float* d_log_lut;        /* [log_lut_entries], null until is_ctx_set_ground_model */
    int log_lut_entries;
    /* ring of pinned staging slots: a call blocks the host only when the slot it wants is still
     * being read by the H2D copy of the call IS_STAGE_SLOTS calls ago */
    float* h_ground_pinned[IS_STAGE_SLOTS];
    int* h_vhor_pinned[IS_STAGE_SLOTS];
    is_instance_buffers* h_inst_pinned[IS_STAGE_SLOTS]; /* [max_batch] per-image output arrays */
    hipEvent_t staging_free[IS_STAGE_SLOTS]; /* recorded after the H2D copies of the slot's call */
    bool staging_pending[IS_STAGE_SLOTS];
    int stage_next;
    hipStream_t aux_streams[IS_AUX_STREAMS]; /* column groups of the pairwise DP in flight */
    hipEvent_t ev_fork;
    hipEvent_t ev_joins[IS_AUX_STREAMS];
    int32_t* d_cluster_scratch; /* [max_batch][8][2][C*S] work arrays of k_cluster_instances */
    is_instance_buffers* d_inst_tbl; /* [max_batch] device copy of the caller's per-image arrays */
    int* d_inst_cnt;            /* [max_batch*C][8] instance candidates per column and class */
    unsigned long long* d_counters; /* [IS_CNT_N] evaluation counters (is_set_eval_counters) */
    bool counting;
    /* scratch */
    RowRec* d_recs;          /* [max_batch*C][H+1] */
    float* d_lutT;           /* [max_batch*C][H+1][D] */
    float* d_lutC;           /* [max_batch*C][ceil(H/32)][D] the LUT's block carries of a walk call (CallPlan::lut_carry) */
    int* h_lutf_repairs = nullptr; /* pinned + mapped: calls whose fused LUT hand-over was repaired (DevParams::lutf_repairs) */
    PriorRec* d_priors;      /* [max_batch][H] */
    StepRec* d_steps;        /* [max_batch*C][H]   per-vB transition records of the pairwise DP (64 B) */
    float* d_part_cost;      /* [max_batch*C][3][64] merged partial minima of the current tile */
    int* d_part_idx;         /* [max_batch*C][3][64] */
    float* d_sv;             /* [max_batch*C][2][H+1] compact S / V prefixes */
    float* d_t8row;          /* [max_batch*C][H] pw * (smallest p field) of every StepRec (lemma L8) */
    float* d_blksum;         /* [max_batch*C][ntiles*IS_QPT+1][24] bound-block summaries of the pairwise DP (lemmas L7, L8) */
    float* d_cost_table;     /* [max_batch*C][H][3] */
    int32_t* d_index_table;  /* [max_batch*C][H][3] */
    size_t scratch_bytes;
    /* parameter sweeps (is_compute_sweep, is_recluster): the object slack of ctx_init before the weights decide
     * whether it counts (+inf: a non-finite table or IS_NO_PRUNE), and buffers that grow with the number of sets, owned
     * apart from `owned` (sweep_reserve replaces them) */
    float sigma_od_free;
    PruneRec* d_sweep_prune;            /* [n_sets][columns of the call] the sets' PruneRecs (k_prune_scale) */
    size_t sweep_prune_cap;             /* records */
    is_instance_buffers* d_sweep_inst;  /* [n_sets][n_images] device copy of the caller's per-image arrays */
    is_instance_buffers* h_sweep_inst;  /* pinned staging of the same */
    size_t sweep_inst_cap;              /* entries */
    hipEvent_t sweep_inst_free;         /* recorded behind the H2D copy out of h_sweep_inst */
    bool sweep_inst_pending;
    int* d_sweep_state;                 /* [0] the generic-column count of the call (k_sweep_state), [1] the constant 1 */
    /* timing */
    bool timing;
    hipEvent_t ev[4];
    bool ev_valid;
};

static int ilog2_exact(int n) {
    int l = 0;
    while ((1 << l) < n) l++;
    return l;
}

/* Runs the enclosed calls on the context's device and puts the caller's current device back. */
struct DeviceScope {
    int prev = -1, want;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int device) : want(device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != want) {
            err = hipSetDevice(want);
            switched = err == hipSuccess;
        }
    }
    ~DeviceScope() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define ON_CTX_DEVICE(c)                                                         \
    DeviceScope dev_scope__((c)->device);                                        \
    if (dev_scope__.err != hipSuccess)                                           \
        return fail_hip(dev_scope__.err, "hipSetDevice(ctx->device)", __FILE__, __LINE__)

const char* is_last_error(void) { return g_err; }
const char* is_version(void) { return "instance_stixels_amd-core 0.3 (gfx950)"; }

int is_device_malloc(void** ptr, size_t bytes) { HIP_TRY(hipMalloc(ptr, bytes)); return IS_OK; }
int is_device_free(void* ptr) { HIP_TRY(hipFree(ptr)); return IS_OK; }
int is_host_malloc(void** ptr, size_t bytes) { HIP_TRY(hipHostMalloc(ptr, bytes)); return IS_OK; }
int is_host_free(void* ptr) { HIP_TRY(hipHostFree(ptr)); return IS_OK; }
int is_get_device(int* device) {
    if (!device) return fail_arg("null pointer");
    HIP_TRY(hipGetDevice(device));
    return IS_OK;
}
int is_set_device(int device) { HIP_TRY(hipSetDevice(device)); return IS_OK; }
int is_ctx_device(const is_ctx* ctx) { return ctx ? ctx->device : -1; }
int is_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return IS_OK;
}
int is_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return IS_OK;
}
int is_memcpy2d_d2h(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                    void* stream) {
    HIP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return IS_OK;
}
int is_memset(void* dst, int value, size_t bytes, void* stream) {
    HIP_TRY(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
    return IS_OK;
}
int is_stream_synchronize(void* stream) { HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); return IS_OK; }
int is_device_synchronize(void) { HIP_TRY(hipDeviceSynchronize()); return IS_OK; }
int is_stream_create(void** stream, int blocking) {
    if (!stream) return fail_arg("null pointer");
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, blocking ? hipStreamDefault : hipStreamNonBlocking));
    *stream = (void*)s;
    return IS_OK;
}
int is_stream_destroy(void* stream) {
    if (stream) HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return IS_OK;
}

size_t is_scratch_bytes(const is_ctx* ctx) { return ctx ? ctx->scratch_bytes : 0; }

static int ctx_init(is_ctx* c, const is_stixel_params* p, const float* obj_cost_lut,
                    const float* obj_disparity_range, int max_batch, int device, int P2, int P2S);

int is_ctx_create(const is_stixel_params* p, const float* obj_cost_lut,
                  const float* obj_disparity_range, int max_batch, int device, is_ctx** out_ctx) {
    if (!p || !obj_cost_lut || !obj_disparity_range || !out_ctx) return fail_arg("null pointer");
    if (max_batch < 1) return fail_arg("max_batch < 1");
    if (p->column_step != IS_DOWNSAMPLE_FACTOR)
        return fail_arg("column_step must be 8 (assert at StixelsKernels.cu:318)");
    if (p->rows < 8 || p->rows % 8 != 0) return fail_arg("rows must be a positive multiple of 8");
    if (p->rows * 3 + 2 >= 32768) return fail_arg("rows too large for the int16 index convention");
    if (p->max_dis < 2 || p->max_dis > 1024) return fail_arg("max_dis out of range [2, 1024]");
    if (p->segmentation_classes != 19 || p->segmentation_channels != 21)
        return fail_arg("the class model is Cityscapes: 19 classes + 2 offset channels (Cityscapes.h)");
    if (p->cols < 1) return fail_arg("cols (realcols) < 1");
    if (p->max_sections < 2) return fail_arg("max_sections < 2");
    const int P2 = 1 << ilog2_exact(p->rows + 1);
    const int P2S = 1 << ilog2_exact(p->rows / 8 + 1);
    if (p->rows_power2 != P2 || p->rows_power2_segmentation != P2S)
        return fail_arg("rows_power2 / rows_power2_segmentation inconsistent with rows (Stixels.cu:131-133)");

    /* everything of the context is created on `device`; the caller's current device is put back */
    DeviceScope scope(device);
    if (scope.err != hipSuccess) return fail_hip(scope.err, "hipSetDevice(device)", __FILE__, __LINE__);
    is_ctx* c = (is_ctx*)calloc(1, sizeof(is_ctx));
    if (!c) return IS_ENOMEM;
    const int rc = ctx_init(c, p, obj_cost_lut, obj_disparity_range, max_batch, device, P2, P2S);
    if (rc != IS_OK) { /* release whatever was created; keep the error text of the failure */
        char keep[sizeof(g_err)];
        memcpy(keep, g_err, sizeof(keep));
        is_ctx_destroy(c);
        memcpy(g_err, keep, sizeof(keep));
        return rc;
    }
    *out_ctx = c;
    return IS_OK;
}

/* the branch-and-bound needs non-negative, finite weights (ctx_init; per set of a sweep) */
static bool weights_allow_pruning(float dw, float pw, float sw, float iw) {
    return dw >= 0.0f && sw >= 0.0f && iw >= 0.0f && pw >= 0.0f && dw < IS_FLT_HUGE && sw < IS_FLT_HUGE &&
           iw < IS_FLT_HUGE;
}

static int ctx_init(is_ctx* c, const is_stixel_params* p, const float* obj_cost_lut,
                    const float* obj_disparity_range, int max_batch, int device, int P2, int P2S) {
    c->params = *p;
    c->device = device;
    c->max_batch = max_batch;

    DevParams& d = c->dp;
    d.H = p->rows; d.C = p->cols; d.D = p->max_dis; d.P2 = P2; d.P2S = P2S;
    d.CH = p->segmentation_channels; d.K = p->segmentation_classes; d.S = p->max_sections;
    d.ntiles = (d.H + IS_TILE - 1) / IS_TILE;
    d.log2P2 = ilog2_exact(P2);
    d.invalid = p->invalid_disparity;
    d.pnex_sky_log = p->pnexists_given_sky_log; d.norm_sky = p->normalization_sky;
    d.inv_sigma2_sky = p->inv_sigma2_sky; d.puniform_sky = p->puniform_sky;
    d.nopnex_sky_log = p->nopnexists_given_sky_log;
    d.pnex_gnd_log = p->pnexists_given_ground_log; d.puniform = p->puniform;
    d.nopnex_gnd_log = p->nopnexists_given_ground_log;
    d.dw = p->disparity_weight; d.pw = p->prior_weight; d.sw = p->segmentation_weight;
    d.iw = p->instance_weight;
    d.rows_log = p->rows_log; d.max_dis_log = p->max_dis_log; d.epsilon = p->epsilon;
    d.pgrav = p->pgrav; d.pblg = p->pblg; d.pord = p->pord; d.max_disf = (float)p->max_dis;
    d.log2c = is_logf(2.0f);
    d.nlog07 = -is_logf(0.7f);
    d.nlog03 = -is_logf(0.3f);
    d.nlog_pord = -is_logf(p->pord);
    d.nlog_1mpord = -is_logf(1.0f - p->pord);
    d.first_g = d.log2c + d.rows_log;                       /* StixelsKernels.cu:196-199 */
    d.first_o_below = d.rows_log + d.log2c + d.max_dis_log; /* :189-194 */
    d.first_o_above = d.rows_log + 0.0f + d.max_dis_log;
    d.size_filter = p->clustering_size_filter;
    d.column_step = p->column_step;
    /* the IS_* knobs (experiments, A/B tests) are read here, once per context, never per call */
    const bool no_prune = getenv("IS_NO_PRUNE") != nullptr;
    const bool debug = getenv("IS_DEBUG") != nullptr;
    {
        auto knob = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : -1; };
        Knobs& k = c->knobs;
        k.pw_groups = knob("IS_PW_GROUPS");
        k.p2_split = knob("IS_P2_SPLIT");
        k.p2x = knob("IS_P2X");
        k.win_tiles = knob("IS_P1_WIN_TILES");
        k.lut_fused = knob("IS_LUT_FUSED"); /* the LUT units inside the unary DP launch (is_k_unary_fast.hip, LUTF) */
        k.unary_path = knob("IS_UNARY_PATH"); /* the unary DP of the visited rows only (k_unary_path) */
        d.lutf_wrong_xcc = k.lut_fused >= 2 ? 1 : 0;
        c->last_unary_path = -1;
        c->last_lut_carry_lds = -1;
    }
    {
        /* branch-and-bound constants (PruneRec, is_device.h).  gamma_d bounds the relative error of
         * a prefix computed by a summation tree of depth d: Blelloch needs <= 2 log2(P2) additions
         * on a path, the object LUT's carry chain H/32 + 5; a generous d covers both. */
        const double depth = 2.0 * ilog2_exact(P2) + (double)d.H / 32.0 + 8.0;
        const double gamma = 1.01 * depth * 0x1p-24;
        d.gamma2 = (float)(2.0 * gamma * 1.001);
        double max_abs = 0.0, min_v = 0.0;
        bool finite = true;
        for (size_t i = 0; i < (size_t)d.D * d.D; i++) {
            const double v = obj_cost_lut[i];
            if (!(fabs(v) < 1e30)) finite = false; /* also catches NaN */
            if (fabs(v) > max_abs) max_abs = fabs(v);
            if (v < min_v) min_v = v;
        }
        const bool weights_ok = weights_allow_pruning(d.dw, d.pw, d.sw, d.iw);
        c->sigma_od_free = finite && !no_prune ? (float)(((0.0 - min_v) * d.H + 2.0 * gamma * d.H * max_abs) * 1.001)
                                               : __builtin_inff();
        d.sigma_od = weights_ok ? c->sigma_od_free : __builtin_inff(); /* (+inf: pruning off) */
    }

    /* waves per DP workgroup: the LUT tile is 64*(D+1) floats; keep >= 16 waves per CU */
    c->nwaves_unary = IS_UNARY_WAVES;
    c->nwaves_pairwise = IS_UNARY_WAVES;
    if (sizeof(int) * (6 * (size_t)d.H + 3 * (size_t)d.S + 4) > 160 * 1024 ||
        isk_unary_lds_bytes(&d) > 160 * 1024 || isk_pairwise_lds_bytes(&d, c->nwaves_pairwise) > 160 * 1024 ||
        isk_prepare_lds_bytes(&d) > 160 * 1024 || isk_lut_carry_lds_bytes(&d) > 160 * 1024 ||
        isk_phase2_lds_bytes(&d) > 64 * 1024 ||
        isk_phase2s_lds_bytes(&d) > 64 * 1024 || /* (both far below: no attribute is set for them) */
        sizeof(int) * (size_t)d.C * IS_INSTANCE_CLASSES + 16 > 160 * 1024)
        return fail_arg("shape needs more than 160 KiB of LDS per workgroup");

    const size_t H = d.H, C = d.C, D = d.D, B = max_batch;
    size_t total = 0;
#define ALLOC(ptr, bytes)                                     \
    do {                                                      \
        HIP_TRY(c->owned.alloc(&(ptr), (bytes)));             \
        total += (bytes);                                     \
    } while (0)
    ALLOC(c->d_obj_cost_lut, sizeof(float) * D * D);
    ALLOC(c->d_obj_cost_fn, sizeof(float) * D * D);
    ALLOC(c->d_odr, sizeof(float) * D);
    ALLOC(c->d_rcp, sizeof(float) * (H + 1));
    ALLOC(c->d_col_flags, sizeof(int) * B * C);
    ALLOC(c->d_prune, sizeof(PruneRec) * B * C);
    ALLOC(c->d_n_generic, sizeof(int));
    HIP_TRY(hipMemset(c->d_n_generic, 0, sizeof(int))); /* later calls: k_backtrace clears it */
    ALLOC(c->d_path_bad, 2 * sizeof(int));
    HIP_TRY(hipMemset(c->d_path_bad, 0, 2 * sizeof(int))); /* [0]: k_backtrace clears it */
    c->stage_off_inst = sizeof(float) * B * 3 * H; /* (H is a multiple of 8: 8-byte aligned) */
    c->stage_off_vhor = c->stage_off_inst + sizeof(is_instance_buffers) * B;
    c->stage_bytes = c->stage_off_vhor + sizeof(int) * B;
    ALLOC(c->d_stage, c->stage_bytes);
    c->d_ground = (float*)c->d_stage;
    c->d_inst_tbl = (is_instance_buffers*)(c->d_stage + c->stage_off_inst);
    c->d_vhor = (int*)(c->d_stage + c->stage_off_vhor);
    ALLOC(c->d_recs, sizeof(RowRec) * B * C * (H + 1));
    ALLOC(c->d_lutT, sizeof(float) * B * C * (H + 1) * D);
    ALLOC(c->d_lutC, sizeof(float) * B * C * isk_lut_carry_rows((int)H) * D);
    ALLOC(c->d_priors, sizeof(PriorRec) * B * H);
    ALLOC(c->d_steps, (size_t)64 * B * C * H);
    /* phase 1 may use up to IS_PW_MAX_SPLIT workgroups per column while columns are few */
    const size_t part_slots = (B * C > (size_t)IS_PW_SPLIT_TARGET_WGS ? B * C : (size_t)IS_PW_SPLIT_TARGET_WGS) +
                              (size_t)IS_PW_MAX_SPLIT;
    ALLOC(c->d_part_cost, sizeof(float) * part_slots * 3 * 64);
    ALLOC(c->d_part_idx, sizeof(int) * part_slots * 3 * 64);
    ALLOC(c->d_sv, sizeof(float) * B * C * 2 * (H + 1));
    ALLOC(c->d_t8row, sizeof(float) * B * C * H);
    ALLOC(c->dp.lut_ready, sizeof(int) * B * C);
    HIP_TRY(hipMemset(c->dp.lut_ready, 0, sizeof(int) * B * C));
    ALLOC(c->dp.lutf_bad, sizeof(int));
    HIP_TRY(hipMemset(c->dp.lutf_bad, 0, sizeof(int)));
    HIP_TRY(hipHostMalloc((void**)&c->h_lutf_repairs, sizeof(int), hipHostMallocMapped));
    *c->h_lutf_repairs = 0;
    HIP_TRY(hipHostGetDevicePointer((void**)&c->dp.lutf_repairs, c->h_lutf_repairs, 0));
    ALLOC(c->dp.win_lo, sizeof(int) * B * C * (size_t)c->dp.ntiles);
    HIP_TRY(hipMemset(c->dp.win_lo, 0, sizeof(int) * B * C * (size_t)c->dp.ntiles));
    ALLOC(c->d_blksum, sizeof(float) * B * C * ((size_t)d.ntiles * IS_QPT + 1) * 24);
    ALLOC(c->d_cost_table, sizeof(float) * B * C * H * 3);
    ALLOC(c->d_index_table, sizeof(int32_t) * B * C * H * 3);
    ALLOC(c->d_cluster_scratch, sizeof(int32_t) * B * IS_INSTANCE_CLASSES * 2 * C * (size_t)d.S);
    ALLOC(c->d_inst_cnt, sizeof(int) * B * C * IS_INSTANCE_CLASSES);
    ALLOC(c->d_counters, sizeof(unsigned long long) * IS_CNT_N);
    ALLOC(c->d_sweep_state, 2 * sizeof(int));
    {
        const int init[2] = {0, 1};
        HIP_TRY(hipMemcpy(c->d_sweep_state, init, sizeof(init), hipMemcpyHostToDevice));
    }
#undef ALLOC
    c->scratch_bytes = total;
    for (int i = 0; i < IS_STAGE_SLOTS; i++) {
        HIP_TRY(hipHostMalloc((void**)&c->h_stage[i], c->stage_bytes));
        memset(c->h_stage[i], 0, c->stage_bytes);
        c->h_ground_pinned[i] = (float*)c->h_stage[i];
        c->h_inst_pinned[i] = (is_instance_buffers*)(c->h_stage[i] + c->stage_off_inst);
        c->h_vhor_pinned[i] = (int*)(c->h_stage[i] + c->stage_off_vhor);
        HIP_TRY(hipEventCreateWithFlags(&c->staging_free[i], hipEventDisableTiming));
    }
    for (int i = 0; i < IS_AUX_STREAMS; i++) {
        HIP_TRY(hipStreamCreateWithFlags(&c->aux_streams[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_joins[i], hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->sweep_inst_free, hipEventDisableTiming));
    for (int i = 0; i < 4; i++) HIP_TRY(hipEventCreate(&c->ev[i]));

    {
        /* device copy is TRANSPOSED ([dis][fn]): a wave of 64 consecutive fn reads one row */
        float* t = (float*)malloc(sizeof(float) * D * D);
        for (size_t fn = 0; fn < D; fn++)
            for (size_t dis = 0; dis < D; dis++) t[dis * D + fn] = obj_cost_lut[fn * D + dis];
        hipError_t e = hipMemcpy(c->d_obj_cost_lut, t, sizeof(float) * D * D, hipMemcpyHostToDevice);
        free(t);
        HIP_TRY(e);
    }
    HIP_TRY(hipMemcpy(c->d_obj_cost_fn, obj_cost_lut, sizeof(float) * D * D, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_odr, obj_disparity_range, sizeof(float) * D, hipMemcpyHostToDevice));
    {
        /* inverse_height = (float)(1./(vT+1-vB)) (StixelsKernels.cu:485, 608) doubles as the
         * reciprocal of the exact-division trick; both definitions must agree bit for bit */
        float* t = (float*)malloc(sizeof(float) * (H + 1));
        t[0] = 0.0f;
        bool same = true;
        for (size_t h = 1; h <= H; h++) {
            const float inverse_height = (float)(1. / (double)h);
            t[h] = 1.0f / (float)h;
            same = same && (t[h] == inverse_height);
        }
        hipError_t e = hipMemcpy(c->d_rcp, t, sizeof(float) * (H + 1), hipMemcpyHostToDevice);
        free(t);
        HIP_TRY(e);
        if (!same) return fail_arg("internal: (float)(1./h) != 1.0f/h for some h <= rows");
    }
    HIP_TRY(isk_set_lds_prepare(&d));
    HIP_TRY(isk_set_lds_lut_carry(&d));
    HIP_TRY(isk_set_lds_unary(&d));
    HIP_TRY(isk_set_lds_unary_path(&d));
    HIP_TRY(isk_set_lds_pairwise(&d, c->nwaves_pairwise));
    HIP_TRY(isk_set_lds_backtrace(&d));
    if (debug)
        fprintf(stderr, "[is_core] unary DP: %d waves/WG, %zu B LDS/WG, occupancy API: %d WG/CU\n",
                c->nwaves_unary, isk_unary_lds_bytes(&d), isk_debug_occupancy(&d, c->nwaves_unary));
    return IS_OK;
}

int is_ctx_destroy(is_ctx* c) {
    if (!c) return IS_OK;
    DeviceScope scope(c->device);
    (void)hipDeviceSynchronize();
    c->owned.free_all();
    if (c->h_lutf_repairs) (void)hipHostFree(c->h_lutf_repairs);
    for (int i = 0; i < IS_STAGE_SLOTS; i++) {
        if (c->h_stage[i]) (void)hipHostFree(c->h_stage[i]);
        if (c->staging_free[i]) (void)hipEventDestroy(c->staging_free[i]);
    }
    for (int i = 0; i < IS_AUX_STREAMS; i++) {
        if (c->aux_streams[i]) (void)hipStreamDestroy(c->aux_streams[i]);
        if (c->ev_joins[i]) (void)hipEventDestroy(c->ev_joins[i]);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->sweep_inst_free) (void)hipEventDestroy(c->sweep_inst_free);
    if (c->d_log_lut) (void)hipFree(c->d_log_lut);
    if (c->d_sweep_prune) (void)hipFree(c->d_sweep_prune);
    if (c->d_sweep_inst) (void)hipFree(c->d_sweep_inst);
    if (c->h_sweep_inst) (void)hipHostFree(c->h_sweep_inst);
    for (int i = 0; i < 4; i++)
        if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    free(c);
    return IS_OK;
}

int is_join_columns(is_ctx* c, const float* d_big, int full_cols, int median_join, float* d_joined,
                    int n_images, void* stream) {
    if (!c || !d_big || !d_joined) return fail_arg("null pointer");
    if (n_images < 1) return fail_arg("n_images < 1");
    const is_stixel_params& p = c->params;
    if (p.column_step > 16) return fail_arg("column_step > 16");
    if (p.width_margin + p.cols * p.column_step > full_cols)
        return fail_arg("full_cols smaller than width_margin + realcols*column_step");
    ON_CTX_DEVICE(c);
    HIP_TRY(isk_launch_join(d_big, d_joined, p.rows, full_cols, p.cols, p.column_step,
                            p.width_margin, median_join, p.invalid_disparity, n_images,
                            (hipStream_t)stream));
    return IS_OK;
}

int is_cluster_instances(is_ctx* c, const is_instance_buffers* ib, void* stream) {
    if (!c || !ib) return fail_arg("null pointer");
    if (!ib->d_labels || !ib->d_centerofmass || !ib->d_core_candidates || !ib->d_instances_per_class)
        return fail_arg("d_labels, d_centerofmass, d_core_candidates and d_instances_per_class are required");
    ON_CTX_DEVICE(c);
    /* (the scratch of image slot 0: calls on one context must be stream-ordered, see the header) */
    HIP_TRY(isk_launch_cluster(c->dp.C * c->dp.S, c->params.clustering_eps, c->params.clustering_min_pts,
                               1, nullptr, ib, c->d_cluster_scratch, (hipStream_t)stream));
    return IS_OK;
}

int is_pack_sections(const is_section* d_sections, int n_columns, int max_sections, int32_t* d_counts,
                     int32_t* d_offsets, is_section* d_packed, void* stream) {
    if (!d_sections || !d_counts || !d_offsets || !d_packed) return fail_arg("null pointer");
    if (n_columns < 1 || max_sections < 2) return fail_arg("empty shape");
    if ((((uintptr_t)d_sections) | ((uintptr_t)d_packed)) & 15) return fail_arg("section arrays must be 16-byte aligned");
    HIP_TRY(isk_launch_pack(d_sections, n_columns, max_sections, d_counts, d_offsets, d_packed,
                            (hipStream_t)stream));
    return IS_OK;
}

int is_unpack_sections(const int32_t* d_counts, int32_t* d_offsets, const is_section* d_packed,
                       int n_columns, int max_sections, is_section* d_sections, void* stream) {
    if (!d_sections || !d_counts || !d_offsets || !d_packed) return fail_arg("null pointer");
    if (n_columns < 1 || max_sections < 2) return fail_arg("empty shape");
    if ((((uintptr_t)d_sections) | ((uintptr_t)d_packed)) & 15) return fail_arg("section arrays must be 16-byte aligned");
    HIP_TRY(isk_launch_unpack(d_counts, d_offsets, d_packed, n_columns, max_sections, d_sections,
                              (hipStream_t)stream));
    return IS_OK;
}

int is_flip_and_pad(const float* d_cnn_out, int32_t* d_segmentation, int n_images, int channels,
                    int rows8, int cols8, int rows_power2_segmentation, void* stream) {
    if (!d_cnn_out || !d_segmentation) return fail_arg("null pointer");
    if (n_images < 1 || channels < 1 || rows8 < 1 || cols8 < 1) return fail_arg("empty shape");
    if (rows_power2_segmentation < rows8 + 1 ||
        (rows_power2_segmentation & (rows_power2_segmentation - 1)) != 0)
        return fail_arg("rows_power2_segmentation must be a power of two > rows/8 (Stixels.cu:132-133)");
    HIP_TRY(isk_launch_flip_and_pad(d_cnn_out, d_segmentation, n_images, channels, rows8, cols8,
                                    rows_power2_segmentation, (hipStream_t)stream));
    return IS_OK;
}

/* ---- road estimation (is_k_road.hip) ---- */
/* the frame shape of both entries (max_dis ints of LDS per histogram row); the batched one adds its own row limit */
static bool road_shape_ok(int rows, int cols, int max_dis) {
    return rows >= 1 && cols >= 1 && max_dis >= 1 && max_dis <= 16384;
}

int is_road_vdisparity(const float* d_disparity, int rows, int cols, int max_dis, float threshold,
                       int* d_vdisp, int* d_maximum, uint8_t* d_binary, void* stream) {
    if (!d_disparity || !d_vdisp || !d_maximum || !d_binary) return fail_arg("null pointer");
    if (!road_shape_ok(rows, cols, max_dis)) return fail_arg("bad shape");
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_maximum, 0, sizeof(int), s));
    HIP_TRY(isk_launch_road_vdisparity_single(d_disparity, d_vdisp, d_binary, d_maximum, rows, cols, max_dis,
                                              threshold, s));
    return IS_OK;
}

struct is_road_ctx {
    OwnedBlocks owned;          /* every device block below */
    int device, rows, cols, max_dis, max_batch;
    int numangle, numrho, band; /* Hough accumulator (numangle + 2) x (numrho + 2); angles per workgroup */
    float rho, theta;
    int last_n;                 /* frames of the last is_road_vdisparity_batch (0: none yet) */
    float* d_tab;               /* [2][numangle]: tabSin, tabCos of HoughLines */
    float* d_tab_theta;         /* [2][numangle]: sinf, cosf of the lines' theta = 0.0f + n * theta (is_road_choose_batch) */
    int* d_vdisp;               /* [max_batch][rows][max_dis] */
    uint8_t* d_binary;          /* [max_batch][rows][max_dis] */
    int* d_counters;            /* [max_batch][isk_road_counters()]: maximum, non-zero pixels */
    int* d_points;              /* [max_batch][rows * max_dis]: (i << 16) | j of the non-zero pixels */
    int* d_ncand;               /* [max_batch] */
    int2* d_cand;               /* [max_batch][IS_ROAD_MAX_CANDIDATES]: (accumulator index, votes) */
};

static void road_ctx_free(is_road_ctx* c) {
    c->owned.free_all();
    free(c);
}

int is_road_ctx_create(is_road_ctx** out, int rows, int cols, int max_dis, int max_batch, int device) {
    if (!out) return fail_arg("null pointer");
    *out = nullptr;
    if (!road_shape_ok(rows, cols, max_dis) || rows > 32767) /* (the point list packs (row << 16) | column) */
        return fail_arg("bad shape (rows in [1, 32767], cols >= 1, max_dis in [1, 16384])");
    if (max_batch < 1 || max_batch > 65535) return fail_arg("max_batch outside [1, 65535]");
    if (isk_road_sort_max() != IS_ROAD_MAX_CANDIDATES) return fail_arg("is_k_road.hip and the header disagree");
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    DeviceScope dev_scope(device);
    if (dev_scope.err != hipSuccess) return fail_hip(dev_scope.err, "hipSetDevice(device)", __FILE__, __LINE__);
    /* the geometry and tables of RoadEstimation::HoughLines(image, rows, max_dis, rho, theta, threshold) */
    const float rho = IS_ROAD_HOUGH_RHO, theta = IS_ROAD_HOUGH_THETA;
    const int numangle = is_hough_numangle(theta), numrho = is_hough_numrho(max_dis, rows, rho);
    float* tab = (float*)malloc(sizeof(float) * 4 * numangle); /* [tabSin | tabCos | sinf | cosf of a line's theta] */
    if (!tab) return IS_ENOMEM;
    is_hough_tables(numangle, rho, theta, tab, tab + numangle);
    /* what RoadEstimation::ComputeCameraProperties evaluates for a line of angle index n (k_road_sort writes theta as
     * exactly this expression): the device has no sinf / cosf with libm's bits, so the host's travel */
    for (int n = 0; n < numangle; n++) {
        const float line_theta = 0.0f + n * theta;
        tab[2 * numangle + n] = sinf(line_theta);
        tab[3 * numangle + n] = cosf(line_theta);
    }
    /* angles per workgroup: as many accumulator rows (plus the two halo rows) as 160 KiB of LDS hold */
    const size_t row_bytes = sizeof(int) * (size_t)(numrho + 2);
    int band = (int)(160 * 1024 / row_bytes) - 2;
    if (band > numangle) band = numangle;
    if (band < 1) { free(tab); return fail_arg("Hough accumulator rows do not fit the LDS (rows + max_dis too large)"); }
    const hipError_t e = isk_set_lds_road_hough((int)(row_bytes * (band + 2)));
    if (e != hipSuccess) { free(tab); return fail_hip(e, "isk_set_lds_road_hough", __FILE__, __LINE__); }

    is_road_ctx* c = (is_road_ctx*)calloc(1, sizeof(is_road_ctx));
    if (!c) { free(tab); return IS_ENOMEM; }
    c->device = device; c->rows = rows; c->cols = cols; c->max_dis = max_dis; c->max_batch = max_batch;
    c->numangle = numangle; c->numrho = numrho; c->band = band; c->rho = rho; c->theta = theta;
    const size_t cells = (size_t)rows * max_dis;
    const size_t B = (size_t)max_batch;
    hipError_t err = hipSuccess; /* (the first failure stops the allocations) */
    auto alloc = [&](auto** p, size_t bytes) { if (err == hipSuccess) err = c->owned.alloc(p, bytes); };
    alloc(&c->d_tab, sizeof(float) * 2 * numangle);
    alloc(&c->d_tab_theta, sizeof(float) * 2 * numangle);
    alloc(&c->d_vdisp, sizeof(int) * B * cells);
    alloc(&c->d_binary, B * cells);
    alloc(&c->d_counters, sizeof(int) * B * isk_road_counters());
    alloc(&c->d_points, sizeof(int) * B * cells);
    alloc(&c->d_ncand, sizeof(int) * B);
    alloc(&c->d_cand, sizeof(int2) * B * IS_ROAD_MAX_CANDIDATES);
    if (err == hipSuccess) err = hipMemcpy(c->d_tab, tab, sizeof(float) * 2 * numangle, hipMemcpyHostToDevice);
    if (err == hipSuccess)
        err = hipMemcpy(c->d_tab_theta, tab + 2 * numangle, sizeof(float) * 2 * numangle, hipMemcpyHostToDevice);
    free(tab);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        road_ctx_free(c);
        snprintf(g_err, sizeof(g_err), "is_road_ctx_create: device allocation of %zu frames failed", B);
        return IS_ENOMEM;
    }
    *out = c;
    return IS_OK;
}

int is_road_ctx_destroy(is_road_ctx* c) {
    if (!c) return IS_OK;
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    road_ctx_free(c);
    return IS_OK;
}

int is_road_ctx_device(const is_road_ctx* c) { return c ? c->device : -1; }
const uint8_t* is_road_ctx_binary(const is_road_ctx* c) { return c ? c->d_binary : nullptr; }

int is_road_vdisparity_batch(is_road_ctx* c, const float* d_disparity, int n_images, float threshold,
                             int* d_vdisp, int* d_maximum, uint8_t* d_binary, void* stream) {
    if (!c || !d_disparity) return fail_arg("null pointer");
    if (n_images < 1 || n_images > c->max_batch) return fail_arg("n_images outside [1, max_batch]");
    ON_CTX_DEVICE(c);
    const hipStream_t s = (hipStream_t)stream;
    const int nc = isk_road_counters();
    const size_t cells = (size_t)c->rows * c->max_dis;
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(int) * nc * n_images, s));
    HIP_TRY(isk_launch_road_vdisparity(d_disparity, c->d_vdisp, c->d_binary, c->d_counters, c->d_points, n_images,
                                       c->rows, c->cols, c->max_dis, threshold, s));
    if (d_vdisp)
        HIP_TRY(hipMemcpyAsync(d_vdisp, c->d_vdisp, sizeof(int) * cells * n_images, hipMemcpyDeviceToDevice, s));
    if (d_maximum) /* entry 0 of each frame's counters */
        HIP_TRY(hipMemcpy2DAsync(d_maximum, sizeof(int), c->d_counters, sizeof(int) * nc, sizeof(int), n_images,
                                 hipMemcpyDeviceToDevice, s));
    if (d_binary) HIP_TRY(hipMemcpyAsync(d_binary, c->d_binary, cells * n_images, hipMemcpyDeviceToDevice, s));
    c->last_n = n_images;
    return IS_OK;
}

int is_road_hough_batch(is_road_ctx* c, int n_images, int threshold, int max_lines, int max_candidates,
                        float* d_lines, int* d_votes, int* d_total, int* d_overflow, void* stream) {
    if (!c || !d_lines || !d_total || !d_overflow) return fail_arg("null pointer");
    if (n_images < 1 || n_images > c->last_n)
        return fail_arg("n_images outside [1, frames of the last is_road_vdisparity_batch]");
    if (max_lines < 1) return fail_arg("max_lines < 1");
    if (max_candidates < 1 || max_candidates > IS_ROAD_MAX_CANDIDATES)
        return fail_arg("max_candidates outside [1, IS_ROAD_MAX_CANDIDATES]");
    ON_CTX_DEVICE(c);
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(c->d_ncand, 0, sizeof(int) * n_images, s));
    HIP_TRY(isk_launch_road_hough(c->d_points, c->d_counters, c->d_ncand, c->d_tab, c->d_cand, d_lines, d_votes,
                                  d_total, d_overflow, n_images, c->rows * c->max_dis, c->numangle, c->numrho,
                                  c->band, threshold, max_candidates, max_lines, c->rho, c->theta, s));
    return IS_OK;
}

int is_road_choose_batch(is_road_ctx* c, int n_images, const float* d_lines, const int* d_total, const int* d_overflow,
                         int max_lines, float cy, float baseline, float focal, float min_pitch, float max_pitch,
                         is_road_params fallback, is_road_params* d_road, uint8_t* d_status, void* stream) {
    if (!c || !d_lines || !d_total || !d_overflow || !d_road || !d_status) return fail_arg("null pointer");
    if (n_images < 1 || n_images > c->max_batch) return fail_arg("n_images outside [1, max_batch]");
    if (max_lines < 1) return fail_arg("max_lines < 1");
    ON_CTX_DEVICE(c);
    HIP_TRY(isk_launch_road_choose(d_lines, d_total, d_overflow, c->d_tab_theta, d_road, d_status, n_images, max_lines,
                                   c->numangle, c->theta, c->rows, cy, baseline, focal, min_pitch, max_pitch, fallback,
                                   (hipStream_t)stream));
    return IS_OK;
}

/* ---- f5: render + score (is_k_render.hip) ---- */
int is_section_instance_labels(const is_instance_buffers* per_image, int n_images, int realcols, int max_sections,
                               int32_t* d_section_instance, void* stream) {
    if (!per_image || !d_section_instance) return fail_arg("null pointer");
    if (n_images < 1 || realcols < 1 || max_sections < 1) return fail_arg("empty shape");
    for (int i = 0; i < n_images; i++)
        if (!per_image[i].d_indices || !per_image[i].d_labels || !per_image[i].d_instances_per_class)
            return fail_arg("d_indices, d_labels and d_instances_per_class are required for every image");
    const hipStream_t s = (hipStream_t)stream;
    const size_t cs = (size_t)realcols * max_sections;
    HIP_TRY(hipMemsetAsync(d_section_instance, 0xff, sizeof(int32_t) * cs * n_images, s));
    const int chunk = isk_render_scatter_images();
    for (int i = 0; i < n_images; i += chunk)
        HIP_TRY(isk_launch_section_instance(per_image + i, n_images - i < chunk ? n_images - i : chunk, i, realcols,
                                            max_sections, d_section_instance, s));
    return IS_OK;
}

/* ---- f5 .. f9: what the entry points that read a batch's Sections check alike.  Each calls it where its own sequence
 * of refusals has always had these checks: of two faults at once, the same one still answers. ---- */
/* The frame geometry (is_world_args has no cols and checks its own): the shape, then the entry point's own limit on
 * it (`own`: its message where the limit is broken, else NULL), then max_sections.  NULL: sound. */
template <class A>
static const char* geometry_fault(const A* a, const char* own = nullptr) {
    if (a->n_images < 1 || a->realcols < 1 || a->rows < 1 || a->cols < a->realcols)
        return "bad shape (n_images >= 1, realcols >= 1, rows >= 1, cols >= realcols)";
    if (own) return own;
    if (a->max_sections < 1 || a->max_sections > 32767) return "max_sections outside [1, 32767]";
    return nullptr;
}
/* one of the pointers (a NULL passes) is not a multiple of `bytes`, a power of two */
template <class... P> static bool misaligned(uintptr_t bytes, P... p) { return ((... | (uintptr_t)p) & (bytes - 1)) != 0; }
/* Cityscapes trainId -> labelId (cityscapesscripts' labels.py, trainId2label[c].id): the default table of
 * is_render_sections and is_cnn_label_maps */
static const uint8_t kCityscapesLabel[19] = {7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33};

int is_render_sections(const is_render_args* a, void* stream) {
    if (!a || !a->d_sections) return fail_arg("null sections");
    if (const char* fault = geometry_fault(a)) return fail_arg(fault);
    if ((a->realcols + 64) / 64 > 65535 || (size_t)a->n_images * ((a->rows + 127) / 128) > 0x7fffffff)
        return fail_arg("batch too large for one launch");
    if (misaligned(16, a->d_sections)) return fail_arg("d_sections must be 16-byte aligned");
    if (!a->d_confusion != !a->d_gt_label) return fail_arg("d_confusion and d_gt_label go together");
    if (a->d_confusion && (a->n_labels < 1 || a->n_labels > IS_RENDER_MAX_LABELS))
        return fail_arg("n_labels outside [1, IS_RENDER_MAX_LABELS]");
    if (!a->d_disp_abs_sum != !a->d_disp_count || !a->d_disp_abs_sum != !a->d_gt_disparity)
        return fail_arg("d_gt_disparity, d_disp_abs_sum and d_disp_count go together");
    if (a->h_class_to_label && (a->n_classes < 1 || a->n_classes > IS_RENDER_MAX_CLASSES))
        return fail_arg("n_classes outside [1, IS_RENDER_MAX_CLASSES]");
    uint8_t table[IS_RENDER_MAX_CLASSES] = {0};
    const uint8_t* src = a->h_class_to_label ? a->h_class_to_label : kCityscapesLabel;
    const int n_classes = a->h_class_to_label ? a->n_classes : (int)sizeof(kCityscapesLabel);
    memcpy(table, src, n_classes);
    HIP_TRY(isk_launch_render(a, table, n_classes, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f6: instance overlap tables (is_k_instance_eval.hip) ---- */
int is_instance_overlap(const is_instance_overlap_args* a, void* stream) {
    if (!a || !a->d_sections || !a->d_gt_instance) return fail_arg("null sections or gt");
    if (!a->d_records || !a->d_n_records || !a->d_overflow) return fail_arg("null output");
    const bool large = (long long)a->rows * a->cols > IS_OVERLAP_MAX_CAPACITY;
    if (const char* fault = geometry_fault(a, large ? "frame larger than IS_OVERLAP_MAX_CAPACITY pixels" : nullptr))
        return fail_arg(fault);
    if (a->capacity < 1 || a->capacity > IS_OVERLAP_MAX_CAPACITY) return fail_arg("capacity outside [1, IS_OVERLAP_MAX_CAPACITY]");
    if (a->n_images > 65535 || (a->realcols + 64) / 64 > 65535 || (size_t)a->n_images * ((a->rows + 127) / 128) > 0x7fffffff)
        return fail_arg("batch too large for one launch");
    if (misaligned(16, a->d_sections)) return fail_arg("d_sections must be 16-byte aligned");
    if (misaligned(4, a->d_gt_instance, a->d_section_instance, a->d_n_records, a->d_overflow))
        return fail_arg("d_gt_instance, d_section_instance, d_n_records and d_overflow must be 4-byte aligned");
    if (misaligned(8, a->d_records)) return fail_arg("d_records must be 8-byte aligned");
    HIP_TRY(isk_launch_instance_overlap(a, (hipStream_t)stream));
    return IS_OK;
}

int is_pack_overlap_records(const is_overlap_record* d_records, const int32_t* d_n_records, int n_images,
                            int capacity, is_overlap_record* d_packed, void* stream) {
    if (!d_records || !d_n_records || !d_packed) return fail_arg("null pointer");
    if (n_images < 1 || n_images > 65535 || capacity < 1 || capacity > IS_OVERLAP_MAX_CAPACITY)
        return fail_arg("n_images outside [1, 65535] or capacity outside [1, IS_OVERLAP_MAX_CAPACITY]");
    if (((uintptr_t)d_records | (uintptr_t)d_packed) & 7) return fail_arg("records must be 8-byte aligned");
    if ((uintptr_t)d_n_records & 3) return fail_arg("d_n_records must be 4-byte aligned");
    HIP_TRY(isk_launch_pack_overlap(d_records, d_n_records, n_images, capacity, d_packed, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f7: the stixel world (is_k_world.hip) ---- */
int is_stixel_world(const is_world_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (a->n_images < 1 || a->realcols < 1 || a->rows < 1 || a->column_step < 1)
        return fail_arg("bad shape (n_images >= 1, realcols >= 1, rows >= 1, column_step >= 1)");
    if (a->max_sections < 2 || a->max_sections > 32767) return fail_arg("max_sections outside [2, 32767]");
    if ((long long)a->n_images * a->realcols * a->max_sections > 0x7fffffffLL)
        return fail_arg("n_images * realcols * max_sections does not fit 31 bits");
    if (a->capacity < 0) return fail_arg("negative capacity");
    if (!a->d_sections || !a->d_counts || !a->d_offsets || !a->d_frame_totals) return fail_arg("null sections or output");
    if (!a->h_alpha_ground || !a->h_vhor) return fail_arg("null road parameters");
    if (a->capacity > 0 && !a->d_world) return fail_arg("null d_world with a capacity");
    if (misaligned(16, a->d_sections, a->d_world)) return fail_arg("d_sections and d_world must be 16-byte aligned");
    if (misaligned(4, a->d_section_instance, a->d_counts, a->d_offsets, a->d_frame_totals))
        return fail_arg("d_section_instance, d_counts, d_offsets and d_frame_totals must be 4-byte aligned");
    HIP_TRY(isk_launch_world(a, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f8: instance ids from the ground truth (is_k_assign_gt.hip) ---- */
int is_assign_instances_gt(const is_assign_gt_args* a, void* stream) {
    if (!a || !a->d_sections || !a->d_gt_instance) return fail_arg("null sections or gt");
    if (!a->d_section_instance) return fail_arg("null d_section_instance");
    if (const char* fault = geometry_fault(a)) return fail_arg(fault);
    if ((long long)a->rows * (a->cols / a->realcols) > 0x7fffffffLL)
        return fail_arg("rows * (cols / realcols) does not fit 31 bits");
    if ((long long)a->n_images * ((a->realcols + 3) / 4) > 0x7fffffffLL) return fail_arg("batch too large for one launch");
    if (misaligned(16, a->d_sections)) return fail_arg("d_sections must be 16-byte aligned");
    if (misaligned(4, a->d_gt_instance, a->d_section_instance, a->d_section_votes))
        return fail_arg("d_gt_instance, d_section_instance and d_section_votes must be 4-byte aligned");
    if (a->min_fraction != a->min_fraction) return fail_arg("min_fraction is NaN");
    /* Cityscapes labelIds of trainIds 11..18 (cityscapes_instance_loader.py:45) */
    static const int kCityscapes[IS_INSTANCE_CLASSES] = {24, 25, 26, 27, 28, 31, 32, 33};
    int ids[IS_INSTANCE_CLASSES];
    for (int i = 0; i < IS_INSTANCE_CLASSES; i++) {
        ids[i] = a->gt_is_train_ids ? IS_FIRST_INSTANCE_CLASS + i : a->h_label_ids ? a->h_label_ids[i] : kCityscapes[i];
        if (ids[i] < 0 || ids[i] > 2147482) return fail_arg("label id outside [0, 2147482]");
    }
    is_assign_gt_args r = *a;
    if (r.min_fraction == 0.0) r.min_fraction = 0.1;
    HIP_TRY(isk_launch_assign_gt(&r, ids, (hipStream_t)stream));
    return IS_OK;
}

int is_pack_section_labels(const int32_t* d_section_instance, int n_images, int realcols, int max_sections,
                           int capacity, int32_t* d_packed, void* stream) {
    if (!d_section_instance || !d_packed) return fail_arg("null pointer");
    if (n_images < 1 || realcols < 1 || max_sections < 1 || capacity < 0) return fail_arg("empty shape or negative capacity");
    if ((long long)n_images * realcols * max_sections > 0x7fffffffLL)
        return fail_arg("n_images * realcols * max_sections does not fit 31 bits");
    if ((uintptr_t)d_section_instance & 3) return fail_arg("d_section_instance must be 4-byte aligned");
    if ((uintptr_t)d_packed & 15) return fail_arg("d_packed must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_packed, 0, 16, s));
    HIP_TRY(isk_launch_pack_section_labels(d_section_instance, n_images, realcols, max_sections, capacity, d_packed, s));
    return IS_OK;
}

/* ---- f10: clustering in (x, y, instance disparity) (is_k_instance_disparity.hip) ---- */
static const char* instance_disparity_fault(const is_instance_disparity_args* a) {
    if (!a) return "null args";
    if (!a->d_sections || !a->d_gt_instance || !a->d_disparity_u8) return "null sections, gt or disparity";
    if (!a->instances || !a->d_scratch) return "null instances or scratch";
    if (a->capacity < 1 || a->capacity > IS_INSTANCE_DISPARITY_KEYS)
        return "capacity outside [1, IS_INSTANCE_DISPARITY_KEYS]";
    if (!(a->eps - a->eps == 0.0f)) return "eps is not finite";
    if (a->min_pts < 1) return "min_pts < 1";
    if (const char* fault = geometry_fault(a, a->n_images > 65535 ? "n_images outside [1, 65535]" : nullptr)) return fault;
    if ((long long)a->realcols * a->max_sections > 0x7fffffffLL) return "realcols * max_sections does not fit 31 bits";
    if ((long long)a->rows * ((a->cols + 7) / 8) > 0x7fffffffLL || (long long)a->rows * (a->cols / a->realcols) > 0x7fffffffLL)
        return "rows * ceil(cols / 8) or rows * (cols / realcols) does not fit 31 bits";
    if ((long long)a->n_images * ((a->realcols + 3) / 4) > 0x7fffffffLL) return "batch too large for one launch";
    if (misaligned(16, a->d_sections, a->d_scratch)) return "d_sections and d_scratch must be 16-byte aligned";
    if (misaligned(4, a->d_gt_instance, a->d_stixel_median, a->d_key_count))
        return "d_gt_instance, d_stixel_median and d_key_count must be 4-byte aligned";
    if (misaligned(2, a->d_key_median)) return "d_key_median must be 2-byte aligned";
    if (a->scratch_bytes < isk_instance_disparity_scratch_bytes(a->n_images, a->realcols, a->max_sections, a->capacity))
        return "scratch_bytes below is_instance_disparity_scratch_bytes()";
    for (int i = 0; i < a->n_images; i++) {
        const is_instance_buffers& ib = a->instances[i];
        if (!ib.d_indices || !ib.d_centerofmass || !ib.d_core_candidates || !ib.d_instances_per_class || !ib.d_labels)
            return "d_indices, d_centerofmass, d_core_candidates, d_instances_per_class and d_labels are required for "
                   "every image";
    }
    return nullptr;
}

size_t is_instance_disparity_scratch_bytes(int n_images, int realcols, int max_sections, int capacity) {
    if (n_images < 1 || n_images > 65535 || realcols < 1 || max_sections < 1 || max_sections > 32767 || capacity < 1 ||
        capacity > IS_INSTANCE_DISPARITY_KEYS || (long long)realcols * max_sections > 0x7fffffffLL)
        return 0;
    return isk_instance_disparity_scratch_bytes(n_images, realcols, max_sections, capacity);
}

int is_cluster_instance_disparity(const is_instance_disparity_args* a, void* stream) {
    if (const char* fault = instance_disparity_fault(a)) return fail_arg(fault);
    HIP_TRY(isk_launch_instance_disparity(a, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f11 .. f16: what the CNN and training entry points check alike, as geometry_fault above: a message, or NULL
 * where all is sound, called where the entry point's own sequence of refusals has always had the check. ---- */
/* The batch and its 1/8-resolution planes: n_images, then the entry point's own condition (`own`: its message where
 * that is broken, else NULL), then the planes' shape, with at most 2^28 cells where the entry point has that limit. */
static const char* planes_fault(int n_images, int rows8, int cols8, bool cell_limit, const char* own = nullptr) {
    if (n_images < 1 || n_images > 65535) return "n_images outside [1, 65535]";
    if (own) return own;
    if (rows8 < 1 || cols8 < 1) return "rows8 and cols8 must be positive";
    if (cell_limit && (long long)rows8 * cols8 > (1LL << 28)) return "more than 2^28 cells per frame";
    return nullptr;
}
static const char* head_dtype_fault(int dtype) {
    if (dtype != IS_HEAD_F32 && dtype != IS_HEAD_F16 && dtype != IS_HEAD_BF16)
        return "dtype is none of IS_HEAD_F32, IS_HEAD_F16, IS_HEAD_BF16";
    return nullptr;
}
static const char* reserved_fault(const int (&reserved)[4]) {
    for (int r : reserved)
        if (r) return "reserved must be 0";
    return nullptr;
}
/* the full-resolution image over planes of rows8 x cols8 cells: cols may end in a margin right of the planes */
static const char* image_fault(int rows, int cols, int rows8, int cols8) {
    if ((long long)rows != 8LL * rows8) return "rows must be 8 * rows8";
    if ((long long)cols < 8LL * cols8) return "cols below 8 * cols8";
    if ((long long)rows * cols > 0x7fffffffLL) return "rows * cols does not fit 31 bits";
    return nullptr;
}
/* a frame's planes reach past its image stride: the input's (`input`: its message), then the gradient's where there
 * is one */
static const char* stride_fault(long long planes, long long stride, const char* input, const void* d_grad,
                                long long grad_stride) {
    if (stride < planes) return input;
    if (d_grad && grad_stride < planes) return "grad_image_stride below the planes of a frame";
    return nullptr;
}
/* the scratch pointer and, with `need`, its size (the entry points that check other pointers in between call twice) */
static const char* scratch_fault(const void* d_scratch, size_t have = 0, size_t need = 0) {
    if (!d_scratch) return "null d_scratch";
    if (misaligned(16, d_scratch)) return "d_scratch must be 16-byte aligned";
    if (have < need) return "scratch_bytes below what the entry point's *_scratch_bytes() returns";
    return nullptr;
}
/* the key capacity a call works with (0 selects min(256, cells)), or 0 where it is out of range */
static int keys_capacity(long long cells, int capacity) {
    const int most = (int)(cells < IS_GT_TARGETS_MAX_CAPACITY ? cells : IS_GT_TARGETS_MAX_CAPACITY);
    if (capacity == 0) return most < 256 ? most : 256;
    return capacity < 1 || capacity > most ? 0 : capacity;
}

/* ---- f11: ground-truth offset targets (is_k_gt_targets.hip) ---- */
/* a frame of 8x8 cells: rows and cols multiples of 8, at most 2^28 cells */
static const char* cells_fault(int n_images, int rows, int cols) {
    if (n_images < 1 || n_images > 65535) return "n_images outside [1, 65535]";
    if (rows < 8 || cols < 8 || rows % 8 != 0 || cols % 8 != 0) return "rows and cols must be multiples of 8, >= 8";
    if ((long long)(rows / 8) * (cols / 8) > (1LL << 28)) return "more than 2^28 cells per frame";
    if ((long long)n_images * (rows / 8) * ((cols / 8 + 63) / 64) > 0x7fffffffLL) return "batch too large for one launch";
    return nullptr;
}

int is_mode_downsample(const void* d_src, int dtype, int n_images, int rows, int cols, void* d_dst, void* stream) {
    if (!d_src || !d_dst) return fail_arg("null pointer");
    if (dtype != IS_DTYPE_UINT8 && dtype != IS_DTYPE_UINT16 && dtype != IS_DTYPE_INT32)
        return fail_arg("dtype is none of IS_DTYPE_UINT8, IS_DTYPE_UINT16, IS_DTYPE_INT32");
    if (const char* fault = cells_fault(n_images, rows, cols)) return fail_arg(fault);
    const uintptr_t element = dtype == IS_DTYPE_INT32 ? 4 : dtype == IS_DTYPE_UINT16 ? 2 : 1;
    if (misaligned(element, d_src, d_dst)) return fail_arg("d_src and d_dst must be aligned to their element");
    HIP_TRY(isk_launch_mode_downsample(d_src, dtype, n_images, rows / 8, cols / 8, d_dst, (hipStream_t)stream));
    return IS_OK;
}

size_t is_gt_targets_scratch_bytes(int n_images, int rows, int cols, int with_disparity, int capacity) {
    if (cells_fault(n_images, rows, cols)) return 0;
    const int cap = keys_capacity((long long)(rows / 8) * (cols / 8), capacity);
    return cap ? isk_gt_targets_scratch_bytes(n_images, rows / 8, cols / 8, with_disparity, cap) : 0;
}

int is_gt_instance_targets(const is_gt_targets_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_gt_instance) return fail_arg("null d_gt_instance");
    if (!a->d_targets && !a->d_ids8 && !a->d_segmentation) return fail_arg("no output: d_targets, d_ids8 and d_segmentation are all null");
    if (a->d_targets ? a->target_planes != 2 && a->target_planes != 3 : a->target_planes != 0)
        return fail_arg("target_planes must be 2 or 3 with d_targets, 0 without");
    if (a->target_planes == 3 && !a->d_disparity_u16) return fail_arg("3 target planes need d_disparity_u16");
    if (const char* fault = cells_fault(a->n_images, a->rows, a->cols)) return fail_arg(fault);
    if (a->d_segmentation) {
        const int p2s = a->rows_power2_segmentation;
        if (p2s < a->rows / 8 + 1 || (p2s & (p2s - 1)) != 0)
            return fail_arg("rows_power2_segmentation must be a power of two > rows/8 (Stixels.cu:132-133)");
        if (a->channels != IS_GT_TARGETS_CHANNELS) return fail_arg("channels must be 21 with d_segmentation");
    } else if (a->rows_power2_segmentation != 0 || a->channels != 0) {
        return fail_arg("rows_power2_segmentation and channels must be 0 without d_segmentation");
    }
    const int capacity = keys_capacity((long long)(a->rows / 8) * (a->cols / 8), a->capacity);
    if (!capacity) return fail_arg("capacity outside [1, min(rows/8 * cols/8, IS_GT_TARGETS_MAX_CAPACITY)]");
    if (const char* fault = scratch_fault(a->d_scratch)) return fail_arg(fault);
    if (misaligned(4, a->d_gt_instance, a->d_targets, a->d_ids8, a->d_segmentation, a->d_key_count))
        return fail_arg("d_gt_instance, d_targets, d_ids8, d_segmentation and d_key_count must be 4-byte aligned");
    if (misaligned(2, a->d_disparity_u16)) return fail_arg("d_disparity_u16 must be 2-byte aligned");
    const size_t need = isk_gt_targets_scratch_bytes(a->n_images, a->rows / 8, a->cols / 8, a->d_disparity_u16 != nullptr, capacity);
    if (const char* fault = scratch_fault(a->d_scratch, a->scratch_bytes, need)) return fail_arg(fault);
    HIP_TRY(isk_launch_gt_targets(a, capacity, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f12: offset and disparity training losses (is_k_offset_loss.hip) ---- */
static const char* offset_loss_shape_fault(int n_images, int planes, int rows8, int cols8) {
    return planes_fault(n_images, rows8, cols8, true, planes != 2 && planes != 3 ? "planes must be 2 or 3" : nullptr);
}

size_t is_offset_loss_scratch_bytes(int n_images, int planes, int rows8, int cols8, int capacity) {
    if (offset_loss_shape_fault(n_images, planes, rows8, cols8)) return 0;
    const int cap = keys_capacity((long long)rows8 * cols8, capacity);
    return cap ? isk_offset_loss_scratch_bytes(n_images, planes, rows8, cols8, cap) : 0;
}

int is_offset_loss(const is_offset_loss_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_prediction) return fail_arg("null d_prediction");
    if (!a->d_ids8) return fail_arg("null d_ids8");
    if (!a->d_loss) return fail_arg("null d_loss");
    if (const char* fault = offset_loss_shape_fault(a->n_images, a->planes, a->rows8, a->cols8)) return fail_arg(fault);
    if (a->planes == 3 && !a->d_disparity8_u16) return fail_arg("3 planes need d_disparity8_u16");
    if (a->planes == 2 && a->d_disparity8_u16) return fail_arg("d_disparity8_u16 must be null with 2 planes");
    const long long frame = (long long)a->planes * a->rows8 * a->cols8;
    if (const char* fault = stride_fault(frame, a->prediction_image_stride, "prediction_image_stride below the planes of a frame",
                                         a->d_grad, a->grad_image_stride))
        return fail_arg(fault);
    const int capacity = keys_capacity((long long)a->rows8 * a->cols8, a->capacity);
    if (!capacity) return fail_arg("capacity outside [1, min(rows8 * cols8, IS_GT_TARGETS_MAX_CAPACITY)]");
    if (const char* fault = scratch_fault(a->d_scratch)) return fail_arg(fault);
    if (misaligned(4, a->d_prediction, a->d_ids8, a->d_loss, a->d_terms, a->d_grad, a->d_key_count))
        return fail_arg("d_prediction, d_ids8, d_loss, d_terms, d_grad and d_key_count must be 4-byte aligned");
    if (misaligned(2, a->d_disparity8_u16)) return fail_arg("d_disparity8_u16 must be 2-byte aligned");
    const size_t need = isk_offset_loss_scratch_bytes(a->n_images, a->planes, a->rows8, a->cols8, capacity);
    if (const char* fault = scratch_fault(a->d_scratch, a->scratch_bytes, need)) return fail_arg(fault);
    HIP_TRY(isk_launch_offset_loss(a, capacity, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f13: the CNN's segmentation head (is_k_head.hip) ---- */
int is_segmentation_head(const is_segmentation_head_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_features || !a->d_weight || !a->d_bias) return fail_arg("null d_features, d_weight or d_bias");
    if (!a->d_cnn_out && !a->d_segmentation) return fail_arg("d_cnn_out and d_segmentation are both null");
    if (const char* fault = head_dtype_fault(a->dtype)) return fail_arg(fault);
    if (const char* fault = planes_fault(a->n_images, a->rows8, a->cols8, false)) return fail_arg(fault);
    if (a->K < 8 || a->K % 8) return fail_arg("K must be >= 8 and a multiple of 8");
    if (a->n_classes < 1) return fail_arg("n_classes must be >= 1");
    if (a->n_regression < 0) return fail_arg("n_regression must be >= 0");
    if ((long long)a->n_classes + a->n_regression > IS_HEAD_MAX_CHANNELS)
        return fail_arg("n_classes + n_regression above IS_HEAD_MAX_CHANNELS");
    const int P2S = a->rows_power2_segmentation;
    if (P2S < 1 || (P2S & (P2S - 1))) return fail_arg("rows_power2_segmentation is not a power of two");
    if (P2S <= a->rows8) return fail_arg("rows_power2_segmentation must be >= rows8 + 1");
    if (a->clamp_channel != -1) {
        if (a->clamp_channel < a->n_classes || a->clamp_channel >= a->n_classes + a->n_regression)
            return fail_arg("clamp_channel is neither -1 nor a regression channel");
        if (!(a->clamp_lo <= a->clamp_hi)) return fail_arg("clamp_lo must be <= clamp_hi");
    }
    if (const char* fault = reserved_fault(a->reserved)) return fail_arg(fault);
    if (misaligned(a->dtype == IS_HEAD_F32 ? 4 : 2, a->d_features)) return fail_arg("d_features must be aligned to its element");
    if (misaligned(4, a->d_weight, a->d_bias, a->d_cnn_out, a->d_segmentation))
        return fail_arg("d_weight, d_bias, d_cnn_out and d_segmentation must be 4-byte aligned");
    HIP_TRY(isk_launch_segmentation_head(a, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f14: the head's backward pass and the semantic NLL loss (is_k_head_backward.hip, is_k_nll.hip) ---- */
static const char* head_backward_shape_fault(int n_images, int K, int rows8, int cols8, int n_classes, long long channels) {
    if (const char* fault = planes_fault(n_images, rows8, cols8, true)) return fault;
    if (K < 8 || K % 8) return "K must be >= 8 and a multiple of 8";
    if (n_classes < 1) return "n_classes must be >= 1";
    if (channels < n_classes) return "n_regression must be >= 0";
    if (channels > IS_HEAD_MAX_CHANNELS) return "n_classes + n_regression above IS_HEAD_MAX_CHANNELS";
    return nullptr;
}

size_t is_segmentation_head_backward_scratch_bytes(int n_images, int K, int rows8, int cols8, int channels) {
    if (head_backward_shape_fault(n_images, K, rows8, cols8, 1, channels)) return 0;
    return isk_head_backward_scratch_bytes(n_images, K, rows8, cols8, channels);
}

int is_segmentation_head_backward(const is_segmentation_head_backward_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_features || !a->d_weight || !a->d_cnn_out || !a->d_grad_out)
        return fail_arg("null d_features, d_weight, d_cnn_out or d_grad_out");
    if (!a->d_grad_features && !a->d_grad_weight && !a->d_grad_bias && !a->d_grad_logits)
        return fail_arg("d_grad_features, d_grad_weight, d_grad_bias and d_grad_logits are all null");
    if (const char* fault = head_dtype_fault(a->dtype)) return fail_arg(fault);
    const long long CH = (long long)a->n_classes + a->n_regression;
    if (a->n_regression < 0) return fail_arg("n_regression must be >= 0");
    if (const char* fault = head_backward_shape_fault(a->n_images, a->K, a->rows8, a->cols8, a->n_classes, CH))
        return fail_arg(fault);
    if (a->grad_image_stride < CH * a->rows8 * a->cols8) return fail_arg("grad_image_stride below the planes of a frame");
    if (const char* fault = reserved_fault(a->reserved)) return fail_arg(fault);
    const uintptr_t element = a->dtype == IS_HEAD_F32 ? 4 : 2;
    if (misaligned(element, a->d_features, a->d_grad_features))
        return fail_arg("d_features and d_grad_features must be aligned to their element");
    if (misaligned(4, a->d_weight, a->d_cnn_out, a->d_grad_out, a->d_grad_weight, a->d_grad_bias, a->d_grad_logits))
        return fail_arg("d_weight, d_cnn_out, d_grad_out, d_grad_weight, d_grad_bias and d_grad_logits must be 4-byte aligned");
    const size_t need = isk_head_backward_scratch_bytes(a->n_images, a->K, a->rows8, a->cols8, (int)CH);
    if (const char* fault = scratch_fault(a->d_scratch, a->scratch_bytes, need)) return fail_arg(fault);
    HIP_TRY(isk_launch_segmentation_head_backward(a, (hipStream_t)stream));
    return IS_OK;
}

size_t is_semantic_nll_scratch_bytes(int n_images, int rows8, int cols8) {
    if (planes_fault(n_images, rows8, cols8, true) || (long long)n_images * rows8 * cols8 > 0x7fffffffLL) return 0;
    return isk_semantic_nll_scratch_bytes(n_images, rows8, cols8);
}

int is_semantic_nll(const is_semantic_nll_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_cnn_out || !a->d_target) return fail_arg("null d_cnn_out or d_target");
    if (!a->d_loss || !a->d_valid_count || !a->d_bad_count) return fail_arg("null d_loss, d_valid_count or d_bad_count");
    if (a->target_dtype != IS_DTYPE_UINT8 && a->target_dtype != IS_DTYPE_INT32)
        return fail_arg("target_dtype is neither IS_DTYPE_UINT8 nor IS_DTYPE_INT32");
    if (const char* fault = planes_fault(a->n_images, a->rows8, a->cols8, true)) return fail_arg(fault);
    if ((long long)a->n_images * a->rows8 * a->cols8 > 0x7fffffffLL) return fail_arg("n_images * rows8 * cols8 does not fit 31 bits");
    if (a->n_classes < 1 || a->n_classes > IS_HEAD_MAX_CHANNELS) return fail_arg("n_classes outside [1, IS_HEAD_MAX_CHANNELS]");
    const long long planes = (long long)a->n_classes * a->rows8 * a->cols8;
    if (const char* fault = stride_fault(planes, a->cnn_image_stride, "cnn_image_stride below the planes of a frame", a->d_grad,
                                         a->grad_image_stride))
        return fail_arg(fault);
    if (const char* fault = reserved_fault(a->reserved)) return fail_arg(fault);
    if (misaligned(4, a->d_cnn_out, a->d_loss, a->d_valid_count, a->d_bad_count, a->d_grad))
        return fail_arg("d_cnn_out, d_loss, d_valid_count, d_bad_count and d_grad must be 4-byte aligned");
    if (a->target_dtype == IS_DTYPE_INT32 && misaligned(4, a->d_target)) return fail_arg("d_target must be aligned to its element");
    const size_t need = isk_semantic_nll_scratch_bytes(a->n_images, a->rows8, a->cols8);
    if (const char* fault = scratch_fault(a->d_scratch, a->scratch_bytes, need)) return fail_arg(fault);
    HIP_TRY(isk_launch_semantic_nll(a, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f15: the CNN's label maps and their confusion table (is_k_cnn_labels.hip) ---- */
int is_cnn_label_maps(const is_cnn_label_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_cnn_out) return fail_arg("null d_cnn_out");
    if (!a->d_class8 && !a->d_label && !a->d_confusion) return fail_arg("no output: d_class8, d_label and d_confusion are all null");
    if (!a->d_confusion != !a->d_gt_label) return fail_arg("d_confusion and d_gt_label go together");
    if (a->mode != IS_CNN_UP_NEAREST && a->mode != IS_CNN_UP_DECONV)
        return fail_arg("mode is neither IS_CNN_UP_NEAREST nor IS_CNN_UP_DECONV");
    if (const char* fault = planes_fault(a->n_images, a->rows8, a->cols8, false)) return fail_arg(fault);
    if (a->n_classes < 1 || a->n_classes > IS_HEAD_MAX_CHANNELS) return fail_arg("n_classes outside [1, IS_HEAD_MAX_CHANNELS]");
    if (a->channels < a->n_classes) return fail_arg("channels below n_classes");
    if (const char* fault = image_fault(a->rows, a->cols, a->rows8, a->cols8)) return fail_arg(fault);
    if ((long long)a->channels * a->rows8 * a->cols8 > 0x7fffffffLL)
        return fail_arg("channels * rows8 * cols8 does not fit 31 bits");
    if (a->d_confusion && (a->n_labels < 1 || a->n_labels > IS_RENDER_MAX_LABELS))
        return fail_arg("n_labels outside [1, IS_RENDER_MAX_LABELS]");
    if (const char* fault = reserved_fault(a->reserved)) return fail_arg(fault);
    if (misaligned(4, a->d_cnn_out)) return fail_arg("d_cnn_out must be 4-byte aligned");
    if (misaligned(8, a->d_confusion)) return fail_arg("d_confusion must be 8-byte aligned");
    uint8_t table[IS_HEAD_MAX_CHANNELS] = {0};
    if (a->h_class_to_label)
        memcpy(table, a->h_class_to_label, a->n_classes);
    else
        memcpy(table, kCityscapesLabel, sizeof(kCityscapesLabel));
    HIP_TRY(isk_launch_cnn_labels(a, table, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f16: the full-resolution semantic NLL through the `up` layer (is_k_nll_up.hip) ---- */
static const char* semantic_nll_up_shape_fault(int n_images, int rows8, int cols8, int n_classes) {
    if (const char* fault = planes_fault(n_images, rows8, cols8, false)) return fault;
    if (n_classes < 1 || n_classes > IS_HEAD_MAX_CHANNELS) return "n_classes outside [1, IS_HEAD_MAX_CHANNELS]";
    if ((long long)n_classes * rows8 * cols8 > 0x7fffffffLL) return "n_classes * rows8 * cols8 does not fit 31 bits";
    if (64LL * rows8 * cols8 > 0x7fffffffLL) return "rows * cols does not fit 31 bits";
    return nullptr;
}

size_t is_semantic_nll_up_scratch_bytes(int n_images, int rows8, int cols8, int n_classes) {
    if (semantic_nll_up_shape_fault(n_images, rows8, cols8, n_classes)) return 0;
    return isk_semantic_nll_up_scratch_bytes(n_images, rows8, cols8);
}

int is_semantic_nll_up(const is_semantic_nll_up_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_cnn_out || !a->d_target) return fail_arg("null d_cnn_out or d_target");
    if (!a->d_loss || !a->d_valid_count || !a->d_bad_count) return fail_arg("null d_loss, d_valid_count or d_bad_count");
    if (a->mode == IS_CNN_UP_NEAREST)
        return fail_arg("mode IS_CNN_UP_NEAREST: the loss at 1/8 resolution is is_semantic_nll");
    if (a->mode != IS_CNN_UP_DECONV) return fail_arg("mode is not IS_CNN_UP_DECONV");
    if (const char* fault = semantic_nll_up_shape_fault(a->n_images, a->rows8, a->cols8, a->n_classes)) return fail_arg(fault);
    if (const char* fault = image_fault(a->rows, a->cols, a->rows8, a->cols8)) return fail_arg(fault);
    const long long planes = (long long)a->n_classes * a->rows8 * a->cols8;
    if (const char* fault = stride_fault(planes, a->cnn_image_stride, "cnn_image_stride below the planes of a frame", a->d_grad,
                                         a->grad_image_stride))
        return fail_arg(fault);
    if (const char* fault = reserved_fault(a->reserved)) return fail_arg(fault);
    if (misaligned(4, a->d_cnn_out, a->d_loss, a->d_grad)) return fail_arg("d_cnn_out, d_loss and d_grad must be 4-byte aligned");
    if (misaligned(8, a->d_valid_count, a->d_bad_count)) return fail_arg("d_valid_count and d_bad_count must be 8-byte aligned");
    const size_t need = isk_semantic_nll_up_scratch_bytes(a->n_images, a->rows8, a->cols8);
    if (const char* fault = scratch_fault(a->d_scratch, a->scratch_bytes, need)) return fail_arg(fault);
    HIP_TRY(isk_launch_semantic_nll_up(a, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f17, f18, f19: convolution + BatchNorm (+ residual) (+ ReLU) (is_k_conv3x3.hip).  One checker and one launcher:
 * is_conv3x3_* are is_conv_* with kernel = 3 and no residual, is_conv_bn is is_conv_bn_stride with stride = 1. ---- */
static const char* conv_weights_fault(int channels_out, int channels_in, int kernel, int dtype) {
    if (dtype != IS_HEAD_F16 && dtype != IS_HEAD_BF16) return "dtype is neither IS_HEAD_F16 nor IS_HEAD_BF16";
    if (channels_in < 16 || channels_in > 2048 || channels_in % 16) return "channels_in must be a multiple of 16 in [16, 2048]";
    if (channels_out < 32 || channels_out > 2048 || channels_out % 32) return "channels_out must be a multiple of 32 in [32, 2048]";
    if (kernel != 1 && kernel != 3) return "kernel is neither 1 nor 3";
    return nullptr;
}

size_t is_conv_packed_bytes(int channels_out, int channels_in, int kernel, int dtype) {
    if (conv_weights_fault(channels_out, channels_in, kernel, dtype)) return 0;
    return (size_t)channels_out * channels_in * kernel * kernel * 2;
}

int is_conv_pack_weights(const float* d_weight, int channels_out, int channels_in, int kernel, int dtype, void* d_packed,
                         void* stream) {
    if (!d_weight || !d_packed) return fail_arg("null d_weight or d_packed");
    if (const char* fault = conv_weights_fault(channels_out, channels_in, kernel, dtype)) return fail_arg(fault);
    if (misaligned(4, d_weight)) return fail_arg("d_weight must be 4-byte aligned");
    if (misaligned(16, d_packed)) return fail_arg("d_packed must be 16-byte aligned");
    HIP_TRY(isk_launch_conv_pack(d_weight, channels_out, channels_in, kernel, dtype, d_packed, (hipStream_t)stream));
    return IS_OK;
}

/* The one checker and launcher of f17, f18 and f19.  `extents_fault`: the refusal of the caller's own names for the
 * extents (rows8 / cols8 in f17 and f18, rows_in / cols_in in f19). */
static int conv_bn_run(const is_conv_bn_stride_args* a, void* stream, const char* extents_fault) {
    if (!a->d_features || !a->d_packed || !a->d_scale || !a->d_shift || !a->d_out)
        return fail_arg("null d_features, d_packed, d_scale, d_shift or d_out");
    if (const char* fault = conv_weights_fault(a->channels_out, a->channels_in, a->kernel, a->dtype)) return fail_arg(fault);
    if (a->out_dtype != a->dtype && a->out_dtype != IS_HEAD_F32)
        return fail_arg("out_dtype is neither the input's dtype nor IS_HEAD_F32");
    if (a->n_images < 1 || a->n_images > 65535) return fail_arg("n_images outside [1, 65535]");
    if (a->rows_in < 1 || a->rows_in > 32767 || a->cols_in < 1 || a->cols_in > 32767) return fail_arg(extents_fault);
    if (a->stride != 1 && a->stride != 2) return fail_arg("stride is neither 1 nor 2");
    if (a->kernel == 1 && a->dilation != 1) return fail_arg("dilation must be 1 with kernel 1");
    if (a->dilation < 1 || a->dilation > 8) return fail_arg("dilation outside [1, 8]");
    if (a->stride == 2 && a->dilation != 1) return fail_arg("dilation must be 1 with stride 2");
    if (a->relu != 0 && a->relu != 1) return fail_arg("relu must be 0 or 1");
    if (misaligned(16, a->d_packed)) return fail_arg("d_packed must be 16-byte aligned");
    if (misaligned(2, a->d_features)) return fail_arg("d_features must be aligned to its element");
    if (misaligned(2, a->d_residual)) return fail_arg("d_residual must be aligned to its element");
    if (misaligned(a->out_dtype == IS_HEAD_F32 ? 4 : 2, a->d_out)) return fail_arg("d_out must be aligned to its element");
    if (misaligned(4, a->d_scale, a->d_shift)) return fail_arg("d_scale and d_shift must be 4-byte aligned");
    if (a->stride == 2 && a->d_residual == a->d_features)
        return fail_arg("d_residual is d_features with stride 2: the residual has the output's shape, not the features'");
    /* each buffer at its own size (at most 2^16 * 2^11 * 2^30 elements of 4 bytes: no overflow) */
    const uint64_t in_cells = (uint64_t)a->n_images * a->rows_in * a->cols_in;
    const uint64_t out_cells = (uint64_t)a->n_images * ((a->rows_in + a->stride - 1) / a->stride) *
                               ((a->cols_in + a->stride - 1) / a->stride);
    const uint64_t in_bytes = in_cells * a->channels_in * 2, out_bytes = out_cells * a->channels_out * (a->out_dtype == IS_HEAD_F32 ? 4 : 2);
    const uint64_t in0 = (uint64_t)(uintptr_t)a->d_features, out0 = (uint64_t)(uintptr_t)a->d_out;
    if (in0 < out0 + out_bytes && out0 < in0 + in_bytes)
        return fail_arg(a->kernel == 3 ? "d_out overlaps d_features: the halo makes an in-place call wrong"
                                       : "d_out overlaps d_features: other channel groups still read them");
    /* (at stride 1 the residual may be the features themselves: both are only read) */
    const uint64_t res0 = (uint64_t)(uintptr_t)a->d_residual, res_bytes = out_cells * a->channels_out * 2;
    if (a->d_residual && res0 < out0 + out_bytes && out0 < res0 + res_bytes)
        return fail_arg("d_out overlaps d_residual: the kernel reads the residual as memory that the launch does not write");
    /* (last: a call that is refused for this alone has passed every check above) */
    if (const char* fault = reserved_fault(a->reserved)) return fail_arg(fault);
    HIP_TRY(isk_launch_conv_bn(a, (hipStream_t)stream));
    return IS_OK;
}

int is_conv_bn_stride(const is_conv_bn_stride_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    return conv_bn_run(a, stream, "rows_in and cols_in must be in [1, 32767]");
}

int is_conv_bn(const is_conv_bn_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    is_conv_bn_stride_args b = {};
    b.d_features = a->d_features, b.dtype = a->dtype, b.n_images = a->n_images, b.channels_in = a->channels_in;
    b.channels_out = a->channels_out, b.rows_in = a->rows8, b.cols_in = a->cols8, b.kernel = a->kernel, b.stride = 1;
    b.dilation = a->dilation, b.d_packed = a->d_packed, b.d_scale = a->d_scale, b.d_shift = a->d_shift;
    b.d_residual = a->d_residual, b.relu = a->relu, b.d_out = a->d_out, b.out_dtype = a->out_dtype;
    for (int i = 0; i < 4; ++i) b.reserved[i] = a->reserved[i];
    return conv_bn_run(&b, stream, "rows8 and cols8 must be in [1, 32767]");
}

size_t is_conv3x3_packed_bytes(int channels_out, int channels_in, int dtype) {
    return is_conv_packed_bytes(channels_out, channels_in, 3, dtype);
}

int is_conv3x3_pack_weights(const float* d_weight, int channels_out, int channels_in, int dtype, void* d_packed,
                            void* stream) {
    return is_conv_pack_weights(d_weight, channels_out, channels_in, 3, dtype, d_packed, stream);
}

int is_conv3x3_bn_relu(const is_conv3x3_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    is_conv_bn_args b = {};
    b.d_features = a->d_features, b.dtype = a->dtype, b.n_images = a->n_images, b.channels_in = a->channels_in;
    b.channels_out = a->channels_out, b.rows8 = a->rows8, b.cols8 = a->cols8, b.kernel = 3, b.dilation = a->dilation;
    b.d_packed = a->d_packed, b.d_scale = a->d_scale, b.d_shift = a->d_shift, b.d_residual = nullptr, b.relu = a->relu;
    b.d_out = a->d_out, b.out_dtype = a->out_dtype;
    for (int i = 0; i < 4; ++i) b.reserved[i] = a->reserved[i];
    return is_conv_bn(&b, stream);
}

/* ---- f21, f22: the backward pass of is_conv_bn_stride (is_k_conv_backward.hip, is_k_conv_backward_stride.hip).  One
 * checker and one launcher: is_conv_bn_backward is is_conv_bn_stride_backward with stride = 1.  `extents_fault`: the
 * refusal in the caller's own names for the extents (rows8 / cols8 in f21, rows_in / cols_in in f22). ---- */
static const char* conv_backward_shape_fault(int n_images, int channels_in, int channels_out, int rows_in, int cols_in,
                                             int kernel, int stride, int dtype, const char* extents_fault) {
    if (const char* fault = conv_weights_fault(channels_out, channels_in, kernel, dtype)) return fault;
    if (n_images < 1 || n_images > 65535) return "n_images outside [1, 65535]";
    if (rows_in < 1 || rows_in > 32767 || cols_in < 1 || cols_in > 32767) return extents_fault;
    if (stride != 1 && stride != 2) return "stride is neither 1 nor 2";
    if (!isk_conv_backward_scratch_bytes(n_images, channels_in, channels_out, rows_in, cols_in, kernel, stride))
        return "the grid of the weight gradient does not fit 31 bits";
    return nullptr;
}

static const char* const kExtents8 = "rows8 and cols8 must be in [1, 32767]";
static const char* const kExtentsIn = "rows_in and cols_in must be in [1, 32767]";

size_t is_conv_bn_backward_scratch_bytes(int n_images, int channels_in, int channels_out, int rows8, int cols8, int kernel,
                                         int dtype) {
    if (conv_backward_shape_fault(n_images, channels_in, channels_out, rows8, cols8, kernel, 1, dtype, kExtents8)) return 0;
    return isk_conv_backward_scratch_bytes(n_images, channels_in, channels_out, rows8, cols8, kernel, 1);
}

size_t is_conv_bn_stride_backward_scratch_bytes(int n_images, int channels_in, int channels_out, int rows_in, int cols_in,
                                                int kernel, int stride, int dtype) {
    if (conv_backward_shape_fault(n_images, channels_in, channels_out, rows_in, cols_in, kernel, stride, dtype, kExtentsIn))
        return 0;
    return isk_conv_backward_scratch_bytes(n_images, channels_in, channels_out, rows_in, cols_in, kernel, stride);
}

static int conv_bn_backward_run(const is_conv_bn_stride_backward_args* a, void* stream, const char* extents_fault) {
    if (!a->d_features || !a->d_weight || !a->d_scale || !a->d_grad_out)
        return fail_arg("null d_features, d_weight, d_scale or d_grad_out");
    if (!a->d_grad_features && !a->d_grad_weight && !a->d_grad_scale && !a->d_grad_shift && !a->d_grad_pre)
        return fail_arg("d_grad_features, d_grad_weight, d_grad_scale, d_grad_shift and d_grad_pre are all null");
    if (const char* fault = conv_backward_shape_fault(a->n_images, a->channels_in, a->channels_out, a->rows_in, a->cols_in,
                                                      a->kernel, a->stride, a->dtype, extents_fault))
        return fail_arg(fault);
    if (a->kernel == 1 && a->dilation != 1) return fail_arg("dilation must be 1 with kernel 1");
    if (a->dilation < 1 || a->dilation > 8) return fail_arg("dilation outside [1, 8]");
    if (a->stride == 2 && a->dilation != 1) return fail_arg("dilation must be 1 with stride 2");
    if (a->relu != 0 && a->relu != 1) return fail_arg("relu must be 0 or 1");
    if (a->relu && !a->d_out) return fail_arg("null d_out with relu: the mask reads the saved output");
    if (a->relu && a->out_dtype != a->dtype && a->out_dtype != IS_HEAD_F32)
        return fail_arg("out_dtype is neither the input's dtype nor IS_HEAD_F32");
    if (a->grad_out_dtype != a->dtype && a->grad_out_dtype != IS_HEAD_F32)
        return fail_arg("grad_out_dtype is neither the input's dtype nor IS_HEAD_F32");
    if (a->d_grad_features && a->grad_features_dtype != a->dtype && a->grad_features_dtype != IS_HEAD_F32)
        return fail_arg("grad_features_dtype is neither the input's dtype nor IS_HEAD_F32");
    if (a->d_grad_features && a->channels_in % 32)
        return fail_arg("d_grad_features needs channels_in % 32 == 0: it is the transposed call's channels_out");
    if (a->d_grad_features_add && !a->d_grad_features) return fail_arg("d_grad_features_add without d_grad_features");
    /* P: the pixels of an OUTPUT plane; P_in: of an input plane */
    const uint64_t P = (uint64_t)((a->rows_in + a->stride - 1) / a->stride) * ((a->cols_in + a->stride - 1) / a->stride);
    const uint64_t P_in = (uint64_t)a->rows_in * a->cols_in, planes = P * a->channels_out;
    if (a->grad_image_stride < (long long)planes) return fail_arg("grad_image_stride below the planes of a frame");
    const uintptr_t out_el = a->out_dtype == IS_HEAD_F32 ? 4 : 2, gy_el = a->grad_out_dtype == IS_HEAD_F32 ? 4 : 2;
    const uintptr_t dx_el = a->grad_features_dtype == IS_HEAD_F32 ? 4 : 2;
    if (misaligned(2, a->d_features, a->d_grad_features_add, a->d_grad_pre))
        return fail_arg("d_features, d_grad_features_add and d_grad_pre must be aligned to their element");
    if (a->relu && misaligned(out_el, a->d_out)) return fail_arg("d_out must be aligned to its element");
    if (misaligned(gy_el, a->d_grad_out)) return fail_arg("d_grad_out must be aligned to its element");
    if (misaligned(dx_el, a->d_grad_features)) return fail_arg("d_grad_features must be aligned to its element");
    if (misaligned(4, a->d_weight, a->d_scale, a->d_grad_weight, a->d_grad_scale, a->d_grad_shift))
        return fail_arg("d_weight, d_scale, d_grad_weight, d_grad_scale and d_grad_shift must be 4-byte aligned");
    const size_t need = isk_conv_backward_scratch_bytes(a->n_images, a->channels_in, a->channels_out, a->rows_in, a->cols_in,
                                                        a->kernel, a->stride);
    if (const char* fault = scratch_fault(a->d_scratch, a->scratch_bytes, need)) return fail_arg(fault);
    /* every output's bytes against every input's and every other output's, each at its own size (at most 2^16 * 2^11 *
     * 2^30 elements of 4 bytes: no overflow) */
    struct span { const void* p; uint64_t bytes; const char* name; };
    const uint64_t n = a->n_images, wn = (uint64_t)a->channels_out * a->channels_in * a->kernel * a->kernel;
    const uint64_t in_el = n * a->channels_in * P_in;
    const span inputs[] = {
        {a->d_features, in_el * 2, "d_features"},
        {a->d_weight, wn * 4, "d_weight"},
        {a->d_scale, (uint64_t)a->channels_out * 4, "d_scale"},
        {a->relu ? a->d_out : nullptr, n * planes * out_el, "d_out"},
        {a->d_grad_out, ((n - 1) * (uint64_t)a->grad_image_stride + planes) * gy_el, "d_grad_out"},
        {a->d_grad_features_add, in_el * 2, "d_grad_features_add"},
    };
    const span outputs[] = {
        {a->d_grad_features, in_el * dx_el, "d_grad_features"},
        {a->d_grad_weight, wn * 4, "d_grad_weight"},
        {a->d_grad_scale, (uint64_t)a->channels_out * 4, "d_grad_scale"},
        {a->d_grad_shift, (uint64_t)a->channels_out * 4, "d_grad_shift"},
        {a->d_grad_pre, n * planes * 2, "d_grad_pre"},
        {a->d_scratch, need, "d_scratch"},
    };
    auto overlap = [](const span& u, const span& v) {
        const uint64_t u0 = (uint64_t)(uintptr_t)u.p, v0 = (uint64_t)(uintptr_t)v.p;
        return u.p && v.p && u0 < v0 + v.bytes && v0 < u0 + u.bytes;
    };
    for (size_t o = 0; o < sizeof(outputs) / sizeof(outputs[0]); ++o) {
        for (const span& in : inputs)
            if (overlap(outputs[o], in)) return fail_arg("an output's bytes (or the scratch's) overlap an input's");
        for (size_t q = o + 1; q < sizeof(outputs) / sizeof(outputs[0]); ++q)
            if (overlap(outputs[o], outputs[q])) return fail_arg("two outputs' bytes (or an output's and the scratch's) overlap");
    }
    /* (last: a call that is refused for this alone has passed every check above) */
    if (const char* fault = reserved_fault(a->reserved)) return fail_arg(fault);
    HIP_TRY(isk_launch_conv_bn_backward(a, (hipStream_t)stream));
    return IS_OK;
}

int is_conv_bn_stride_backward(const is_conv_bn_stride_backward_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    return conv_bn_backward_run(a, stream, kExtentsIn);
}

int is_conv_bn_backward(const is_conv_bn_backward_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    is_conv_bn_stride_backward_args b = {};
    b.d_features = a->d_features, b.dtype = a->dtype, b.n_images = a->n_images, b.channels_in = a->channels_in;
    b.channels_out = a->channels_out, b.rows_in = a->rows8, b.cols_in = a->cols8, b.kernel = a->kernel, b.stride = 1;
    b.dilation = a->dilation, b.d_weight = a->d_weight, b.d_scale = a->d_scale, b.d_out = a->d_out;
    b.out_dtype = a->out_dtype, b.relu = a->relu, b.d_grad_out = a->d_grad_out, b.grad_out_dtype = a->grad_out_dtype;
    b.grad_image_stride = a->grad_image_stride, b.d_grad_features = a->d_grad_features;
    b.grad_features_dtype = a->grad_features_dtype, b.d_grad_features_add = a->d_grad_features_add;
    b.d_grad_weight = a->d_grad_weight, b.d_grad_scale = a->d_grad_scale, b.d_grad_shift = a->d_grad_shift;
    b.d_grad_pre = a->d_grad_pre, b.d_scratch = a->d_scratch, b.scratch_bytes = a->scratch_bytes;
    for (int i = 0; i < 4; ++i) b.reserved[i] = a->reserved[i];
    return conv_bn_backward_run(&b, stream, kExtents8);
}

/* ---- f20: the backbone's stem, image bytes to layer1's output (is_k_stem.hip).  One checker, one launcher. ---- */
static const char* stem_dtype_fault(int dtype) {
    return dtype != IS_HEAD_F16 && dtype != IS_HEAD_BF16 ? "dtype is neither IS_HEAD_F16 nor IS_HEAD_BF16" : nullptr;
}

size_t is_stem_packed_bytes(int dtype) { return stem_dtype_fault(dtype) ? 0 : isk_stem_packed_bytes(); }

int is_stem_pack_weights(const float* d_w0, const float* d_w1, int dtype, void* d_packed, void* stream) {
    if (!d_w0 || !d_w1 || !d_packed) return fail_arg("null d_w0, d_w1 or d_packed");
    if (const char* fault = stem_dtype_fault(dtype)) return fail_arg(fault);
    if (misaligned(4, d_w0, d_w1)) return fail_arg("d_w0 and d_w1 must be 4-byte aligned");
    if (misaligned(16, d_packed)) return fail_arg("d_packed must be 16-byte aligned");
    HIP_TRY(isk_launch_stem_pack(d_w0, d_w1, dtype, d_packed, (hipStream_t)stream));
    return IS_OK;
}

int is_stem(const is_stem_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_image || !a->d_lut || !a->d_packed || !a->d_scale0 || !a->d_shift0 || !a->d_scale1 || !a->d_shift1 || !a->d_out)
        return fail_arg("null d_image, d_lut, d_packed, d_scale0, d_shift0, d_scale1, d_shift1 or d_out");
    if (const char* fault = stem_dtype_fault(a->dtype)) return fail_arg(fault);
    if (a->n_images < 1 || a->n_images > 65535) return fail_arg("n_images outside [1, 65535]");
    if (a->rows < 1 || a->rows > 32767 || a->cols < 1 || a->cols > 32767) return fail_arg("rows and cols must be in [1, 32767]");
    if (misaligned(16, a->d_packed)) return fail_arg("d_packed must be 16-byte aligned");
    if (misaligned(2, a->d_lut)) return fail_arg("d_lut must be aligned to its element");
    if (misaligned(2, a->d_mid)) return fail_arg("d_mid must be aligned to its element");
    if (misaligned(2, a->d_out)) return fail_arg("d_out must be aligned to its element");
    if (misaligned(4, a->d_scale0, a->d_shift0, a->d_scale1, a->d_shift1))
        return fail_arg("d_scale0, d_shift0, d_scale1 and d_shift1 must be 4-byte aligned");
    /* each buffer at its own size (at most 2^16 * 2^30 pixels of 32 bytes: no overflow) */
    const uint64_t pixels = (uint64_t)a->n_images * a->rows * a->cols, image_bytes = pixels * 3, plane_bytes = pixels * 16 * 2;
    const uint64_t image0 = (uint64_t)(uintptr_t)a->d_image, out0 = (uint64_t)(uintptr_t)a->d_out, mid0 = (uint64_t)(uintptr_t)a->d_mid;
    if (a->d_mid && mid0 < out0 + plane_bytes && out0 < mid0 + plane_bytes) return fail_arg("d_out overlaps d_mid");
    if (image0 < out0 + plane_bytes && out0 < image0 + image_bytes)
        return fail_arg("d_out overlaps d_image: other workgroups still read the image");
    if (a->d_mid && image0 < mid0 + plane_bytes && mid0 < image0 + image_bytes)
        return fail_arg("d_mid overlaps d_image: other workgroups still read the image");
    /* (last: a call that is refused for this alone has passed every check above) */
    if (const char* fault = reserved_fault(a->reserved)) return fail_arg(fault);
    HIP_TRY(isk_launch_stem(a, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f23: the backward pass of the stem (is_k_stem_backward.hip).  One checker, one launcher. ---- */
static const char* stem_backward_shape_fault(int n_images, int rows, int cols, int channels_next, int dtype) {
    if (const char* fault = stem_dtype_fault(dtype)) return fault;
    if (n_images < 1 || n_images > 65535) return "n_images outside [1, 65535]";
    if (rows < 1 || rows > 32767 || cols < 1 || cols > 32767) return "rows and cols must be in [1, 32767]";
    if (channels_next != 0 && (channels_next < 32 || channels_next > 128 || channels_next % 32))
        return "channels_next must be a multiple of 32 in [32, 128]";
    return nullptr;
}

size_t is_stem_backward_scratch_bytes(int n_images, int rows, int cols, int channels_next, int dtype) {
    if (stem_backward_shape_fault(n_images, rows, cols, channels_next, dtype)) return 0;
    return isk_stem_backward_scratch_bytes(n_images, rows, cols, channels_next);
}

int is_stem_backward_constant(int which) {
    static const int values[4] = {IS_STEM_BACKWARD_BAND, IS_STEM_BACKWARD_SEGMENT, IS_STEM_BACKWARD_TILE_ROWS,
                                  IS_STEM_BACKWARD_TILE_COLS};
    return which >= 0 && which < 4 ? values[which] : -1;
}

int is_stem_backward(const is_stem_backward_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_image || !a->d_lut || !a->d_w0 || !a->d_w1 || !a->d_scale0 || !a->d_scale1 || !a->d_mid || !a->d_out)
        return fail_arg("null d_image, d_lut, d_w0, d_w1, d_scale0, d_scale1, d_mid or d_out");
    const bool source_b = a->d_grad_next || a->channels_next || a->d_weight_next || a->d_scale_next;
    if (a->d_grad_out && source_b) return fail_arg("both gradient sources: d_grad_out and d_grad_next's fields");
    if (!a->d_grad_out && !source_b) return fail_arg("no gradient source: d_grad_out is null");
    if (source_b && (!a->d_grad_next || !a->d_weight_next || !a->d_scale_next))
        return fail_arg("null d_grad_next, d_weight_next or d_scale_next");
    if (source_b && !a->channels_next) return fail_arg("channels_next must be a multiple of 32 in [32, 128]");
    if (const char* fault = stem_backward_shape_fault(a->n_images, a->rows, a->cols, a->channels_next, a->dtype))
        return fail_arg(fault);
    if (!source_b && a->grad_out_dtype != a->dtype && a->grad_out_dtype != IS_HEAD_F32)
        return fail_arg("grad_out_dtype is neither the stem's dtype nor IS_HEAD_F32");
    const uint64_t P = (uint64_t)a->rows * a->cols, planes = 16 * P;
    const uint64_t P_next = (uint64_t)((a->rows + 1) / 2) * ((a->cols + 1) / 2);
    if (!source_b && a->grad_image_stride < (long long)planes) return fail_arg("grad_image_stride below the planes of a frame");
    const uintptr_t gy_el = a->grad_out_dtype == IS_HEAD_F32 ? 4 : 2;
    if (misaligned(2, a->d_lut, a->d_mid, a->d_out, a->d_grad_pre1, a->d_grad_pre0, a->d_grad_next))
        return fail_arg("d_lut, d_mid, d_out, d_grad_pre1, d_grad_pre0 and d_grad_next must be aligned to their element");
    if (!source_b && misaligned(gy_el, a->d_grad_out)) return fail_arg("d_grad_out must be aligned to its element");
    if (misaligned(4, a->d_w0, a->d_w1, a->d_scale0, a->d_scale1, a->d_weight_next, a->d_scale_next))
        return fail_arg("d_w0, d_w1, d_scale0, d_scale1, d_weight_next and d_scale_next must be 4-byte aligned");
    if (misaligned(4, a->d_grad_weight0, a->d_grad_scale0, a->d_grad_shift0, a->d_grad_weight1, a->d_grad_scale1, a->d_grad_shift1))
        return fail_arg("the fp32 gradients must be 4-byte aligned");
    const size_t need = isk_stem_backward_scratch_bytes(a->n_images, a->rows, a->cols, a->channels_next);
    if (const char* fault = scratch_fault(a->d_scratch, a->scratch_bytes, need)) return fail_arg(fault);
    /* every output's bytes against every input's and every other output's, each at its own size (at most 2^16 * 2^30
     * pixels of 64 bytes: no overflow) */
    struct span { const void* p; uint64_t bytes; };
    const uint64_t n = a->n_images;
    const span inputs[] = {
        {a->d_image, n * P * 3},      {a->d_lut, 3 * 256 * 2},  {a->d_w0, 16 * 3 * 49 * 4}, {a->d_w1, 16 * 16 * 9 * 4},
        {a->d_scale0, 16 * 4},        {a->d_scale1, 16 * 4},    {a->d_mid, n * planes * 2}, {a->d_out, n * planes * 2},
        {a->d_grad_out, source_b ? 0 : ((n - 1) * (uint64_t)a->grad_image_stride + planes) * gy_el},
        {a->d_grad_next, n * a->channels_next * P_next * 2},
        {a->d_weight_next, (uint64_t)a->channels_next * 16 * 9 * 4},
        {a->d_scale_next, (uint64_t)a->channels_next * 4},
    };
    const span outputs[] = {
        {a->d_grad_weight0, 16 * 3 * 49 * 4}, {a->d_grad_scale0, 16 * 4}, {a->d_grad_shift0, 16 * 4},
        {a->d_grad_weight1, 16 * 16 * 9 * 4}, {a->d_grad_scale1, 16 * 4}, {a->d_grad_shift1, 16 * 4},
        {a->d_grad_pre1, n * planes * 2},     {a->d_grad_pre0, n * planes * 2}, {a->d_scratch, need},
    };
    auto overlap = [](const span& u, const span& v) {
        const uint64_t u0 = (uint64_t)(uintptr_t)u.p, v0 = (uint64_t)(uintptr_t)v.p;
        return u.p && v.p && u0 < v0 + v.bytes && v0 < u0 + u.bytes;
    };
    for (size_t o = 0; o < sizeof(outputs) / sizeof(outputs[0]); ++o) {
        for (const span& in : inputs)
            if (overlap(outputs[o], in)) return fail_arg("an output's bytes (or the scratch's) overlap an input's");
        for (size_t q = o + 1; q < sizeof(outputs) / sizeof(outputs[0]); ++q)
            if (overlap(outputs[o], outputs[q])) return fail_arg("two outputs' bytes (or an output's and the scratch's) overlap");
    }
    if (!a->d_grad_weight0 && !a->d_grad_scale0 && !a->d_grad_shift0 && !a->d_grad_weight1 && !a->d_grad_scale1 &&
        !a->d_grad_shift1 && !a->d_grad_pre1 && !a->d_grad_pre0)
        return fail_arg("no output is asked for");
    /* (last: a call that is refused for this alone has passed every check above) */
    if (const char* fault = reserved_fault(a->reserved)) return fail_arg(fault);
    HIP_TRY(isk_launch_stem_backward(a, (hipStream_t)stream));
    return IS_OK;
}

/* ---- f9: per-instance objects and contours (is_k_objects.hip) ---- */
int is_instance_objects(const is_instance_objects_args* a, void* stream) {
    if (!a) return fail_arg("null args");
    if (!a->d_sections) return fail_arg("null sections");
    if (const char* fault = geometry_fault(a, a->n_images > 65535 ? "n_images outside [1, 65535]" : nullptr))
        return fail_arg(fault);
    if ((long long)a->n_images * a->realcols * a->max_sections > 0x7fffffffLL)
        return fail_arg("n_images * realcols * max_sections does not fit 31 bits");
    if (a->object_capacity < 0 || a->point_capacity < 0) return fail_arg("negative capacity");
    if (!a->d_frame_objects || !a->d_frame_points || !a->d_totals) return fail_arg("null output");
    if ((a->object_capacity > 0 && !a->d_objects) || (a->point_capacity > 0 && !a->d_points))
        return fail_arg("null d_objects or d_points with a capacity");
    if (misaligned(16, a->d_sections, a->d_objects, a->d_points))
        return fail_arg("d_sections, d_objects and d_points must be 16-byte aligned");
    if (misaligned(4, a->d_section_instance, a->d_frame_objects, a->d_frame_points, a->d_totals))
        return fail_arg("d_section_instance, d_frame_objects, d_frame_points and d_totals must be 4-byte aligned");
    HIP_TRY(isk_launch_instance_objects(a, (hipStream_t)stream));
    return IS_OK;
}

static_assert(IS_CNT_N == IS_EVAL_COUNTERS, "is_device.h and instance_stixels_core.h disagree on the counter array");

int is_set_eval_counters(is_ctx* c, int enabled) {
    if (!c) return fail_arg("null ctx");
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(c->d_counters, 0, sizeof(unsigned long long) * IS_CNT_N));
    c->counting = enabled != 0;
    return IS_OK;
}

int is_get_eval_counters(is_ctx* c, unsigned long long* out, int n) {
    if (!c || !out) return fail_arg("null pointer");
    if (n < 1 || n > IS_CNT_N) return fail_arg("n outside [1, IS_EVAL_COUNTERS]");
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, c->d_counters, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
    return IS_OK;
}

int is_debug_read_object_lut(is_ctx* c, int column, float* h_out) {
    if (!c || !h_out) return fail_arg("null pointer");
    if (column < 0 || column >= c->max_batch * c->dp.C) return fail_arg("column outside the context's scratch");
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = ((size_t)c->dp.H + 1) * c->dp.D;
    HIP_TRY(hipMemcpy(h_out, c->d_lutT + (size_t)column * n, sizeof(float) * n, hipMemcpyDeviceToHost));
    return IS_OK;
}

int is_debug_read_lut_carries(is_ctx* c, int column, float* h_out) {
    if (!c || !h_out) return fail_arg("null pointer");
    if (column < 0 || column >= c->max_batch * c->dp.C) return fail_arg("column outside the context's scratch");
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = (size_t)isk_lut_carry_rows(c->dp.H) * c->dp.D;
    HIP_TRY(hipMemcpy(h_out, c->d_lutC + (size_t)column * n, sizeof(float) * n, hipMemcpyDeviceToHost));
    return IS_OK;
}

int is_debug_lut_carry_lds(is_ctx* c, int* on, int* pass_columns) {
    if (!c || !on || !pass_columns) return fail_arg("null pointer");
    *on = c->last_lut_carry_lds;
    *pass_columns = isk_lut_carry_pass_columns();
    return IS_OK;
}

int is_debug_lut_fused_state(is_ctx* c, int* repaired) {
    if (!c || !repaired) return fail_arg("null pointer");
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(repaired, c->dp.lutf_bad, sizeof(int), hipMemcpyDeviceToHost));
    return IS_OK;
}

int is_lut_fused_repairs(is_ctx* c, int* calls_repaired) {
    if (!c || !calls_repaired) return fail_arg("null pointer");
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    *calls_repaired = c->h_lutf_repairs ? *(volatile int*)c->h_lutf_repairs : 0;
    return IS_OK;
}

int is_debug_unary_path(is_ctx* c, int* path, int* repaired) {
    if (!c || !path || !repaired) return fail_arg("null pointer");
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    int w[2] = {0, 0};
    HIP_TRY(hipMemcpy(w, c->d_path_bad, sizeof(w), hipMemcpyDeviceToHost));
    *path = c->last_unary_path;
    *repaired = w[1];
    return IS_OK;
}

int is_debug_read_block_summaries(is_ctx* c, int column, float* h_out, int cap_floats, int* n_blocks) {
    if (!c || !h_out || !n_blocks) return fail_arg("null pointer");
    if (column < 0 || column >= c->max_batch * c->dp.C) return fail_arg("column outside the context's scratch");
    const int nb = c->dp.ntiles * IS_QPT + 1;
    if (cap_floats < nb * 24) return fail_arg("h_out too small");
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_out, c->d_blksum + (size_t)column * nb * 24, sizeof(float) * nb * 24, hipMemcpyDeviceToHost));
    *n_blocks = nb;
    return IS_OK;
}

int is_set_kernel_timing(is_ctx* c, int enabled) {
    if (!c) return fail_arg("null ctx");
    c->timing = enabled != 0;
    c->ev_valid = false;
    return IS_OK;
}

int is_get_kernel_times_ms(is_ctx* c, float* prepare_ms, float* dp_ms, float* backtrace_ms) {
    if (!c) return fail_arg("null ctx");
    if (!c->timing || !c->ev_valid) return fail_arg("kernel timing not enabled / no call recorded");
    HIP_TRY(hipEventSynchronize(c->ev[3]));
    float a = 0, b = 0, d = 0;
    HIP_TRY(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
    HIP_TRY(hipEventElapsedTime(&d, c->ev[2], c->ev[3]));
    if (prepare_ms) *prepare_ms = a;
    if (dp_ms) *dp_ms = b;
    if (backtrace_ms) *backtrace_ms = d;
    return IS_OK;
}

/* Every launch decision of one DP call (CallPlan, is_launch.h); the launchers launch what it says.  The choices decide
 * launch geometry and kernel instantiations only, never results. */
/* the smallest horizon of a call's frames as plan_call takes it (at most H) */
static int min_vhor(const int* h_vhor, int n_images, int H) {
    int vmin = H;
    for (int i = 0; i < n_images; i++) vmin = h_vhor[i] < vmin ? h_vhor[i] : vmin;
    return vmin;
}

static CallPlan plan_call(const is_ctx* c, const DevParams& P, int n_images, int pairwise, int vhor_min,
                          bool tables_requested, bool want_inst) {
    const Knobs& k = c->knobs;
    const int ncols = n_images * P.C;
    CallPlan p = {};
    p.ncols = ncols, p.pairwise = pairwise, p.nwaves = pairwise ? c->nwaves_pairwise : c->nwaves_unary;

    /* fn windows (is_device.h, IS_P1_WIN).  Pairwise phase 1: the tiles that start below the horizon of every image of
     * the call -- ground and what stands on it span few disparities within 64 rows, while a tile above the horizon
     * mixes sky (d ~ 0) with objects of any disparity: measured, 3.6 % of the steps of tile 7 read outside the window,
     * 22-35 % of tiles 12-13, and a step with a lane outside pays a memory round trip on a latency-bound chain.  The
     * unary kernel windows EVERY tile: a lane outside costs it an L2 gather (2.8 % of its steps on the synthetic
     * scene) -- measured at batch 64: 9 windowed tiles 7450, all 16: 7760 frames/s (pairwise 3780 / 3810, but its
     * unpruned floor 1720 / 1630).  IS_P1_WIN_TILES forces the window for that many tiles at any call size: tests. */
    if (IS_P1_WINDOWED(P.D) && (k.win_tiles >= 0 || ncols >= (pairwise ? IS_P1_WIN_MIN_COLS : ISF_WIN_MIN_COLS))) {
        int w = k.win_tiles >= 0 ? k.win_tiles : P.ntiles;
        if (k.win_tiles < 0 && pairwise) {
            const int vmin = vhor_min < P.H ? vhor_min : P.H;
            w = vmin > 0 ? (vmin + IS_TILE - 1) / IS_TILE : 0;
        }
        p.win_tiles = w < P.ntiles ? w : P.ntiles;
    }

    if (!pairwise) {
        /* The unary DP along the back-trace's path (k_unary_path, is_k_unary_path.hip): the call computes only the table
         * rows k_backtrace visits instead of every row, and repair launches redo the call on the tile path when a walk
         * meets what it cannot vouch for.  IS_UNARY_PATH:
         *   -1 / unset  automatic: unary calls that request no tables (d_cost_table / d_index_table null), with the
         *               evaluation counters off (they instrument the tile kernels), IS_LUT_FUSED not 2 / 3 (those test
         *               the fused hand-over), pruning on (IS_NO_PRUNE unset, finite weights and object costs: an
         *               unpruned walk is slower than the tile path, measured 2345 against 3040 frames/s) and at least
         *               IS_UNARY_PATH_MIN_COLS columns;
         *    0          never;
         *    1          the same rules at any number of columns;
         *    2          (tests) also when tables are requested: only the visited rows of the caller's tables are written;
         *    3          (tests) as 2, and every call distrusts itself: the repair launches run. */
        if (!c->counting && k.unary_path != 0)
            p.unary_walk = k.unary_path >= 2 ||
                           (!tables_requested && k.lut_fused != 2 && k.lut_fused != 3 && P.sigma_od < IS_FLT_HUGE &&
                            (k.unary_path == 1 || ncols >= IS_UNARY_PATH_MIN_COLS));
        p.unary_force_bad = p.unary_walk && k.unary_path == 3;
        /* the walk knows (vT, vB, type, cost) of every Section when it hops: it writes them, and k_backtrace takes
         * only what the walk left (generic columns, a distrusted call).  Instance outputs need k_backtrace's
         * candidate counts of every column: such calls keep the ungated launch. */
        p.walk_sections = p.unary_walk && !want_inst;
        /* the tile path: FAST columns through the chunk-staged kernel of is_k_unary_fast.hip whenever the shape allows
         * it, then k_dp_unary takes only the generic columns (measured on MI355X, batch 64: 8.7 ms against 9.3 ms of
         * the tile-pair kernel, and no scratch) */
        p.unary_nvr = p.unary_walk ? 0 : isk_unary_fast_chunk_rows(&P);
        /* LUTF: the LUT units run inside the unary DP launch -- every tile windowed in ONE launch of 4-wave workgroups,
         * 1, 2 or 4 units per column (a LUT block is four waves).  By itself only where it pays (ISF_LUTF_MIN_COLS; D =
         * 256, four units per column, 32 frames of 1024x4096: 3940 | 4040 frames/s fused | prepare launch);
         * IS_LUT_FUSED=1 / 2: at any size.  A hand-over of this context that has been distrusted before (another
         * dispatcher, a partition mode, a CU mask) keeps it off unless IS_LUT_FUSED asks for it by value: a repaired
         * call costs 2.8 x an ordinary one. */
        const int fnb = (P.D + 63) / 64;
        const bool by_itself = k.lut_fused < 0 || k.lut_fused == 3; /* (3, tests: the default policy, wrong XCC id) */
        const bool repaired_before = c->h_lutf_repairs && *(volatile int*)c->h_lutf_repairs > 0;
        p.lut_fused = p.unary_nvr != 0 && k.lut_fused != 0 && ISF_WIN_WAVES == 4 && (fnb == 1 || fnb == 2 || fnb == 4) &&
                      p.win_tiles == P.ntiles &&
                      !(by_itself && (ncols < ISF_LUTF_MIN_COLS || fnb > 2 || repaired_before));
    }
    p.prepare_lut = !p.lut_fused;
    /* the walk rebuilds the table entries it reads from the block carries (k_unary_path); the launches behind it that
     * read the complete table build it first for the columns they take (isk_launch_dp_unary) */
    p.lut_carry = p.unary_walk;
    /* ... and builds them from a cost table in LDS where it fits beside a second workgroup (k_lut_carry, D <= 128);
     * other shapes keep the carry units of k_prepare_fused */
    p.lut_carry_lds = p.lut_carry && p.prepare_lut && isk_lut_carry_lds_bytes(&P) != 0;

    if (pairwise) {
        /* few columns: two workgroups per (column, tile) in phase 1 */
        p.nsplit = ncols <= IS_PW_SPLIT_MAX_COLS ? 2 : 1;
        /* Columns are independent: with enough of them the batch is cut into groups whose phase-1 / phase-2 chains
         * (2 x ntiles dependent launches each) run on streams of their own, so that the tails and the latency-bound
         * serial phase 2 of one group share the CUs with the other groups' launches */
        static_assert(IS_PAIRWISE_MAX_GROUPS <= IS_AUX_STREAMS + 1, "a column group needs a stream of the context");
        p.groups = ncols / IS_PAIRWISE_SPLIT_MIN_COLS;
        p.groups = p.groups < 1 ? 1 : p.groups > IS_PAIRWISE_MAX_GROUPS ? IS_PAIRWISE_MAX_GROUPS : p.groups;
        if (k.pw_groups >= 1 && k.pw_groups <= IS_AUX_STREAMS + 1) p.groups = k.pw_groups;
        /* phase 2: four waves per column while the columns are too few to fill the chip (IS_P2_SPLIT_MAX_COLS);
         * large batches two columns per wave (k_pw_phase2x), which needs an even number of columns per image (a pair
         * never straddles two images); IS_P2X=0 selects k_pw_phase2 */
        bool split2 = ncols <= IS_P2_SPLIT_MAX_COLS;
        if (k.p2_split >= 0) split2 = k.p2_split != 0;
        p.phase2 = split2 ? IS_P2_SPLIT
                   : (P.C % 2) == 0 && k.p2x != 0 && isk_phase2x_lds_bytes(&P) <= 64 * 1024 ? IS_P2_TWO : IS_P2_ONE;
    }

    if (ncols <= IS_BACKTRACE_STAGE_MAX_COLS && isk_backtrace_lds_bytes(&P, IS_BT_STAGED) <= 64 * 1024)
        p.backtrace = IS_BT_STAGED;
    else if (ncols >= IS_BACKTRACE_TWO_MIN_COLS && isk_backtrace_lds_bytes(&P, IS_BT_TWO) <= 160 * 1024)
        p.backtrace = IS_BT_TWO;
    else
        p.backtrace = IS_BT_PLAIN;
    return p;
}

/* The H2D copies of a call's staging slot: the ground model and the horizons, with the per-image instance table in
 * the same copy where the batch is full (`inst_tbl`: a call with fewer frames copies the table by itself). */
static int enqueue_staging(is_ctx* c, int n_images, bool inst_tbl, hipStream_t stream, int slot,
                           bool ground = true) {
    const size_t H = c->dp.H;
    if (!ground) { /* is_compute_road: the ground model and the horizons are written on the device */
        if (inst_tbl)
            HIP_TRY(hipMemcpyAsync(c->d_inst_tbl, c->h_inst_pinned[slot], sizeof(is_instance_buffers) * n_images,
                                   hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(c->staging_free[slot], stream));
        return IS_OK;
    }
    const bool one_copy = n_images == c->max_batch;
    if (one_copy) {
        HIP_TRY(hipMemcpyAsync(c->d_stage, c->h_stage[slot], c->stage_bytes, hipMemcpyHostToDevice, stream));
    } else {
        HIP_TRY(hipMemcpyAsync(c->d_ground, c->h_ground_pinned[slot], sizeof(float) * n_images * 3 * H,
                               hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(c->d_vhor, c->h_vhor_pinned[slot], sizeof(int) * n_images,
                               hipMemcpyHostToDevice, stream));
    }
    if (inst_tbl && !one_copy) /* the per-image output pointers travel through the pinned staging slot of this call */
        HIP_TRY(hipMemcpyAsync(c->d_inst_tbl, c->h_inst_pinned[slot], sizeof(is_instance_buffers) * n_images,
                               hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(c->staging_free[slot], stream));
    return IS_OK;
}

/* which outputs the per-image arrays of a call ask for */
static void instance_wants(const is_instance_buffers* instances, int n, bool* want_inst, bool* want_labels) {
    *want_inst = *want_labels = false;
    if (instances)
        for (int i = 0; i < n; i++) {
            const is_instance_buffers& ib = instances[i];
            *want_inst = *want_inst || ib.d_centerofmass || ib.d_indices || ib.d_core_candidates ||
                         ib.d_instances_per_class;
            *want_labels = *want_labels || ib.d_labels;
        }
}

/* the context's scratch as the launchers take it (the caller adds its outputs) */
static CallBuffers call_buffers(const is_ctx* c, const float* d_joined, const int32_t* d_seg) {
    CallBuffers b;
    b.joined = d_joined; b.seg = d_seg; b.ground = c->d_ground; b.vhor = c->d_vhor;
    b.cost_T = c->d_obj_cost_lut; b.cost_F = c->d_obj_cost_fn; b.odr = c->d_odr; b.rcp = c->d_rcp;
    b.recs = c->d_recs; b.lutT = c->d_lutT; b.lutC = c->d_lutC; b.col_flags = c->d_col_flags; b.sv = c->d_sv; b.prune = c->d_prune;
    b.n_generic = c->d_n_generic; b.path_bad = c->d_path_bad; b.priors = c->d_priors; b.steps = c->d_steps;
    b.part_cost = c->d_part_cost; b.part_idx = c->d_part_idx; b.blksum = c->d_blksum; b.t8row = c->d_t8row;
    b.cost_table = c->d_cost_table;
    b.index_table = c->d_index_table;
    b.sections = nullptr;
    b.counters = c->counting ? c->d_counters : nullptr;
    b.inst_cnt = nullptr;
    return b;
}

/* The tail of a DP call behind its prepare launches: the pairwise or unary DP, the back-trace into b.sections and, with
 * instance outputs (b.inst_cnt), the instance candidates (StixelsKernels.cu:926-942) and their clustering
 * (Stixels::ClusterInstances, Stixels.cu:613) of the WHOLE batch into d_tbl: two launches.  ev_dp (timing, or null) is
 * recorded between the DP and the back-trace. */
static int dp_tail_enqueue(is_ctx* c, const DevParams& P, const CallPlan& plan, const CallBuffers& b, int n_images,
                           const is_instance_buffers* d_tbl, bool want_labels, float eps, int min_pts,
                           hipStream_t stream, hipEvent_t ev_dp) {
    if (plan.pairwise)
        HIP_TRY(isk_launch_dp_pairwise(&P, &plan, &b, stream, c->aux_streams, c->ev_fork, c->ev_joins));
    else
        HIP_TRY(isk_launch_dp_unary(&P, &plan, &b, stream));
    if (ev_dp) HIP_TRY(hipEventRecord(ev_dp, stream));
    HIP_TRY(isk_launch_backtrace(&P, &plan, &b, stream));
    if (b.inst_cnt) {
        HIP_TRY(isk_launch_compact(&P, n_images, b.sections, b.inst_cnt, d_tbl, stream));
        if (want_labels)
            HIP_TRY(isk_launch_cluster(P.C * P.S, eps, min_pts, n_images, d_tbl, nullptr, c->d_cluster_scratch, stream));
    }
    return IS_OK;
}

/* Everything is_compute and is_compute_road queue on `stream` behind the host-side staging of slot `slot`.  d_road
 * null (is_compute): the slot's ground model is uploaded.  Else k_ground_model builds it from d_road in place, and
 * the plan takes vhor_min_hint (< 0: unknown, planned as 0) for the smallest horizon. */
static int compute_enqueue(is_ctx* c, const float* d_joined, const int32_t* d_seg, int pairwise, int n_images,
                           is_section* d_sections, const is_instance_buffers* instances, float* d_cost_table,
                           int32_t* d_index_table, hipStream_t stream, int slot,
                           const is_road_params* d_road = nullptr, int vhor_min_hint = -1) {
    const DevParams& P = c->dp;
    const bool timing = c->timing;
    bool want_inst = false, want_labels = false;
    instance_wants(instances, n_images, &want_inst, &want_labels);
    const int rc_stage = enqueue_staging(c, n_images, want_inst, stream, slot, d_road == nullptr);
    if (rc_stage != IS_OK) return rc_stage;
    if (d_road)
        HIP_TRY(isk_launch_ground_model(&c->ground_params, c->d_log_lut, c->log_lut_entries, d_road, c->d_ground,
                                        c->d_vhor, n_images, P.H, stream));

    const int vhor_min = d_road ? (vhor_min_hint < 0 ? 0 : vhor_min_hint) : min_vhor(c->h_vhor_pinned[slot], n_images, P.H);
    const CallPlan plan = plan_call(c, P, n_images, pairwise, vhor_min,
                                    d_cost_table != nullptr || d_index_table != nullptr, want_inst);
    if (!pairwise) c->last_unary_path = plan.unary_walk;
    c->last_lut_carry_lds = plan.lut_carry_lds;
    CallBuffers b = call_buffers(c, d_joined, d_seg);
    if (d_cost_table) b.cost_table = d_cost_table;
    if (d_index_table) b.index_table = d_index_table;
    b.sections = d_sections;
    b.inst_cnt = want_inst ? c->d_inst_cnt : nullptr;

    if (timing) HIP_TRY(hipEventRecord(c->ev[0], stream));
    /* (d_n_generic is zero here: cleared at creation and by k_backtrace at the end of every call; the prepare launch
     * clears d_path_bad[0], the distrust word of the last walk) */
    HIP_TRY(isk_launch_prepare(&P, &plan, &b, stream));
    if (pairwise) HIP_TRY(isk_launch_priors(&P, c->d_ground, c->d_priors, n_images, stream));
    if (timing) HIP_TRY(hipEventRecord(c->ev[1], stream));
    const int rc = dp_tail_enqueue(c, P, plan, b, n_images, c->d_inst_tbl, want_labels, c->params.clustering_eps,
                                   c->params.clustering_min_pts, stream, timing ? c->ev[2] : nullptr);
    if (rc != IS_OK) return rc;
    if (timing) {
        HIP_TRY(hipEventRecord(c->ev[3], stream));
        c->ev_valid = true;
    }
    return IS_OK;
}

/* The argument checks is_compute and is_compute_sweep share (`n_inst` entries of `instances`). */
static const char* compute_fault(const is_ctx* c, const float* d_joined, const int32_t* d_seg, int n_images,
                                 const is_section* d_sections, const is_instance_buffers* instances, long long n_inst) {
    if (!c || !d_joined || !d_seg || !d_sections) return "null pointer";
    if (n_images < 1 || n_images > c->max_batch) return "n_images outside [1, max_batch]";
    if ((((uintptr_t)d_joined) | ((uintptr_t)d_seg)) & 15)
        return "d_joined / d_segmentation must be 16-byte aligned (vector loads)";
    if (instances)
        for (long long i = 0; i < n_inst; i++)
            if (instances[i].d_labels && (!instances[i].d_centerofmass || !instances[i].d_core_candidates ||
                                          !instances[i].d_instances_per_class))
                return "d_labels needs d_centerofmass, d_core_candidates and d_instances_per_class";
    return nullptr;
}

/* The host half of a call: the per-frame ground model (the reference does 3 blocking cudaMemcpy per frame,
 * Stixels.cu:479-493) and the per-image instance table into the next pinned staging slot: pinned + async, through a
 * ring of slots each guarded by an event.  `instances`: n_images entries or NULL. */
static int stage_call(is_ctx* c, const float* h_gf, const float* h_ng, const float* h_is2, const int* h_vhor,
                      int n_images, const is_instance_buffers* instances, int* out_slot) {
    const size_t H = c->dp.H;
    const int slot = c->stage_next;
    c->stage_next = (slot + 1) % IS_STAGE_SLOTS;
    if (c->staging_pending[slot]) HIP_TRY(hipEventSynchronize(c->staging_free[slot]));
    for (int i = 0; h_gf && i < n_images; i++) { /* (h_gf null, is_compute_road: the instance table only) */
        float* dst = c->h_ground_pinned[slot] + (size_t)i * 3 * H;
        memcpy(dst, h_gf + (size_t)i * H, sizeof(float) * H);
        memcpy(dst + H, h_ng + (size_t)i * H, sizeof(float) * H);
        memcpy(dst + 2 * H, h_is2 + (size_t)i * H, sizeof(float) * H);
        c->h_vhor_pinned[slot][i] = h_vhor[i];
    }
    /* (no instances: zeros, so that the one-copy path of a full batch never leaves pointers of an
     * older call -- possibly freed since -- in d_inst_tbl) */
    if (instances) memcpy(c->h_inst_pinned[slot], instances, sizeof(is_instance_buffers) * n_images);
    else memset(c->h_inst_pinned[slot], 0, sizeof(is_instance_buffers) * n_images);
    c->staging_pending[slot] = true;
    *out_slot = slot;
    return IS_OK;
}

/* Invariant the early-outs of k_dp_unary / k_pw_phase2_generic rely on: d_n_generic is zero
 * between calls (k_prepare counts the generic columns of a call, block 0 of k_backtrace clears
 * the counter at its end).  A call that failed half way may have counted without clearing. */
static void clear_call_state(is_ctx* c, hipStream_t stream) {
    (void)hipMemsetAsync(c->d_n_generic, 0, sizeof(int), stream);
    (void)hipMemsetAsync(c->d_path_bad, 0, sizeof(int), stream);
}

int is_compute(is_ctx* c, const float* d_joined, const int32_t* d_seg, const float* h_gf,
               const float* h_ng, const float* h_is2, const int* h_vhor, int pairwise, int n_images,
               is_section* d_sections, const is_instance_buffers* instances, float* d_cost_table,
               int32_t* d_index_table, void* stream_) {
    if (!h_gf || !h_ng || !h_is2 || !h_vhor) return fail_arg("null pointer");
    if (const char* fault = compute_fault(c, d_joined, d_seg, n_images, d_sections, instances, n_images))
        return fail_arg(fault);
    ON_CTX_DEVICE(c);
    hipStream_t stream = (hipStream_t)stream_;
    int slot = 0;
    const int rc_stage = stage_call(c, h_gf, h_ng, h_is2, h_vhor, n_images, instances, &slot);
    if (rc_stage != IS_OK) return rc_stage;
    const int rc = compute_enqueue(c, d_joined, d_seg, pairwise, n_images, d_sections, instances, d_cost_table,
                                   d_index_table, stream, slot);
    if (rc != IS_OK) clear_call_state(c, stream);
    return rc;
}

int is_ctx_set_ground_model(is_ctx* c, const is_ground_params* params, const float* h_log_lut, int n_entries) {
    if (!c || !params || !h_log_lut) return fail_arg("null pointer");
    if (n_entries < 2) return fail_arg("n_entries < 2");
    ON_CTX_DEVICE(c);
    if (n_entries != c->log_lut_entries) {
        HIP_TRY(hipDeviceSynchronize()); /* (a queued call may still read the old table) */
        if (c->d_log_lut) (void)hipFree(c->d_log_lut);
        c->d_log_lut = nullptr;
        c->log_lut_entries = 0;
        HIP_TRY(hipMalloc((void**)&c->d_log_lut, sizeof(float) * (size_t)n_entries));
        c->log_lut_entries = n_entries;
    }
    HIP_TRY(hipMemcpy(c->d_log_lut, h_log_lut, sizeof(float) * (size_t)n_entries, hipMemcpyHostToDevice));
    c->ground_params = *params;
    return IS_OK;
}

int is_compute_road(is_ctx* c, const float* d_joined, const int32_t* d_seg, const is_road_params* d_road, int pairwise,
                    int n_images, is_section* d_sections, const is_instance_buffers* instances, float* d_cost_table,
                    int32_t* d_index_table, int vhor_min_hint, void* stream_) {
    if (!d_road) return fail_arg("null pointer");
    if (const char* fault = compute_fault(c, d_joined, d_seg, n_images, d_sections, instances, n_images))
        return fail_arg(fault);
    if (!c->d_log_lut) return fail_arg("is_compute_road before is_ctx_set_ground_model");
    ON_CTX_DEVICE(c);
    hipStream_t stream = (hipStream_t)stream_;
    int slot = 0;
    const int rc_stage = stage_call(c, nullptr, nullptr, nullptr, nullptr, n_images, instances, &slot);
    if (rc_stage != IS_OK) return rc_stage;
    const int rc = compute_enqueue(c, d_joined, d_seg, pairwise, n_images, d_sections, instances, d_cost_table,
                                   d_index_table, stream, slot, d_road, vhor_min_hint);
    if (rc != IS_OK) clear_call_state(c, stream);
    return rc;
}

int is_debug_read_ground(is_ctx* c, int frame, float* h_out, int* vhor) {
    if (!c || !h_out || !vhor) return fail_arg("null pointer");
    if (frame < 0 || frame >= c->max_batch) return fail_arg("frame outside [0, max_batch)");
    ON_CTX_DEVICE(c);
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = 3 * (size_t)c->dp.H;
    HIP_TRY(hipMemcpy(h_out, c->d_ground + (size_t)frame * n, sizeof(float) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vhor, c->d_vhor + frame, sizeof(int), hipMemcpyDeviceToHost));
    return IS_OK;
}

/* ---- parameter sweeps ---- */

/* The sweep's own buffers for `records` PruneRecs and `entries` instance-table entries: grown into locals, the
 * context's members replaced after both exist (the old ones only after the device has finished with them). */
static int sweep_reserve(is_ctx* c, size_t records, size_t entries) {
    if (records > c->sweep_prune_cap) {
        PruneRec* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, sizeof(PruneRec) * records));
        HIP_TRY(hipDeviceSynchronize());
        if (c->d_sweep_prune) (void)hipFree(c->d_sweep_prune);
        c->d_sweep_prune = p;
        c->sweep_prune_cap = records;
    }
    if (entries > c->sweep_inst_cap) {
        is_instance_buffers *d = nullptr, *h = nullptr;
        HIP_TRY(hipMalloc((void**)&d, sizeof(is_instance_buffers) * entries));
        const hipError_t e = hipHostMalloc((void**)&h, sizeof(is_instance_buffers) * entries);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail_hip(e, "hipHostMalloc(sweep instance table)", __FILE__, __LINE__);
        }
        HIP_TRY(hipDeviceSynchronize());
        if (c->d_sweep_inst) (void)hipFree(c->d_sweep_inst);
        if (c->h_sweep_inst) (void)hipHostFree(c->h_sweep_inst);
        c->d_sweep_inst = d;
        c->h_sweep_inst = h;
        c->sweep_inst_cap = entries;
        c->sweep_inst_pending = false;
    }
    return IS_OK;
}

/* `n` entries of the caller's instance table to d_sweep_inst through the pinned copy, on `stream` */
static int sweep_stage_instances(is_ctx* c, const is_instance_buffers* instances, size_t n, hipStream_t stream) {
    if (c->sweep_inst_pending) HIP_TRY(hipEventSynchronize(c->sweep_inst_free));
    memcpy(c->h_sweep_inst, instances, sizeof(is_instance_buffers) * n);
    HIP_TRY(hipMemcpyAsync(c->d_sweep_inst, c->h_sweep_inst, sizeof(is_instance_buffers) * n, hipMemcpyHostToDevice,
                           stream));
    HIP_TRY(hipEventRecord(c->sweep_inst_free, stream));
    c->sweep_inst_pending = true;
    return IS_OK;
}

/* Everything is_compute_sweep queues on `stream`.  Once: the staging copies, the prepare launch, the pairwise priors
 * (k_prior_tables reads no weight), the sets' PruneRecs.  Per set: what compute_enqueue queues behind its prepare
 * launch, with a DevParams of the set's own.  The per-call state a single call consumes:
 *  - d_n_generic: kept behind the prepare launch and put back in front of every set after the first (k_sweep_state);
 *    k_backtrace of the last set leaves it zero, as the invariant between calls asks;
 *  - d_path_bad[0]: cleared in front of every set after the first by the same launch;
 *  - the object table: the carry rows where a set walks, the complete table where a set takes the tile path, both
 *    where the sets disagree; never the fused LUT + DP launch, whose table would be rebuilt per set;
 *  - d_inst_cnt, d_cluster_scratch, cost / index scratch, the pairwise scratch: one stream, so the sets follow each
 *    other through them as consecutive calls do. */
static int sweep_enqueue(is_ctx* c, const float* d_joined, const int32_t* d_seg, int pairwise, int n_images,
                         const is_sweep_set* sets, int n_sets, is_section* d_sections,
                         const is_instance_buffers* instances, hipStream_t stream, int slot) {
    const int ncols = n_images * c->dp.C;
    const size_t frame_sections = (size_t)c->dp.C * c->dp.S;
    c->ev_valid = false; /* (a sweep records no kernel times: is_get_kernel_times_ms refuses until the next is_compute) */
    const int rc_stage = enqueue_staging(c, n_images, false, stream, slot);
    if (rc_stage != IS_OK) return rc_stage;
    if (instances) {
        const int rc = sweep_stage_instances(c, instances, (size_t)n_sets * n_images, stream);
        if (rc != IS_OK) return rc;
    }

    /* the sets' parameter blocks and plans */
    DevParams* Pk = (DevParams*)malloc(sizeof(DevParams) * n_sets);
    CallPlan* plans = (CallPlan*)malloc(sizeof(CallPlan) * n_sets);
    struct Release { void *a, *b; ~Release() { free(a); free(b); } } release{Pk, plans};
    if (!Pk || !plans) return IS_ENOMEM;
    bool any_walk = false, any_tile = false;
    for (int k = 0; k < n_sets; k++) {
        DevParams& P = Pk[k];
        P = c->dp;
        P.dw = sets[k].disparity_weight; P.pw = sets[k].prior_weight; P.sw = sets[k].segmentation_weight;
        P.iw = sets[k].instance_weight;
        P.size_filter = sets[k].clustering_size_filter;
        P.sigma_od = weights_allow_pruning(P.dw, P.pw, P.sw, P.iw) ? c->sigma_od_free : __builtin_inff();
        bool want_inst = false, want_labels = false;
        instance_wants(instances ? instances + (size_t)k * n_images : nullptr, n_images, &want_inst, &want_labels);
        plans[k] = plan_call(c, P, n_images, pairwise, min_vhor(c->h_vhor_pinned[slot], n_images, P.H), false, want_inst);
        plans[k].lut_fused = 0;
        plans[k].prepare_lut = 1;
        if (!pairwise) (plans[k].unary_walk ? any_walk : any_tile) = true;
    }

    /* the prepare launch with both PruneRec weights 1 and the weight-free object slack: the records it leaves in
     * d_prune are the slacks themselves (is_k_sweep.hip) */
    DevParams P0 = c->dp;
    P0.dw = 1.0f;
    P0.iw = 1.0f;
    P0.sigma_od = c->sigma_od_free;
    CallPlan prep = plans[0];
    prep.lut_carry = any_walk ? 1 : 0;
    prep.lut_carry_lds = prep.lut_carry && isk_lut_carry_lds_bytes(&P0) != 0;
    c->last_lut_carry_lds = prep.lut_carry_lds;
    CallBuffers b = call_buffers(c, d_joined, d_seg);
    HIP_TRY(isk_launch_prepare(&P0, &prep, &b, stream));
    if (any_walk && any_tile) /* the sets disagree: the complete table of every column beside the carry rows */
        HIP_TRY(isk_launch_lut_repair(&P0, ncols, d_joined, c->d_obj_cost_lut, c->d_lutT, c->d_sweep_state + 1, stream));
    if (pairwise) HIP_TRY(isk_launch_priors(&P0, c->d_ground, c->d_priors, n_images, stream));
    for (int k0 = 0; k0 < n_sets; k0 += IS_SWEEP_SCALE_SETS) {
        const int m = n_sets - k0 < IS_SWEEP_SCALE_SETS ? n_sets - k0 : IS_SWEEP_SCALE_SETS;
        SweepScale sc = {};
        for (int k = 0; k < m; k++) {
            sc.dw[k] = Pk[k0 + k].dw;
            sc.iw[k] = Pk[k0 + k].iw;
            sc.sigma_od[k] = Pk[k0 + k].sigma_od;
        }
        HIP_TRY(isk_launch_prune_scale(c->d_prune, c->d_sweep_prune + (size_t)k0 * ncols, ncols, m, &sc, stream));
    }
    HIP_TRY(isk_launch_sweep_state(c->d_n_generic, c->d_path_bad, c->d_sweep_state, 0, stream));

    for (int k = 0; k < n_sets; k++) {
        const DevParams& P = Pk[k];
        const CallPlan& plan = plans[k];
        const is_instance_buffers* inst_k = instances ? instances + (size_t)k * n_images : nullptr;
        const is_instance_buffers* d_tbl = instances ? c->d_sweep_inst + (size_t)k * n_images : nullptr;
        is_section* sections = d_sections + (size_t)k * n_images * frame_sections;
        bool want_inst = false, want_labels = false;
        instance_wants(inst_k, n_images, &want_inst, &want_labels);
        if (k > 0) HIP_TRY(isk_launch_sweep_state(c->d_n_generic, c->d_path_bad, c->d_sweep_state, 1, stream));
        b.prune = c->d_sweep_prune + (size_t)k * ncols;
        b.sections = sections;
        b.inst_cnt = want_inst ? c->d_inst_cnt : nullptr;
        const int rc = dp_tail_enqueue(c, P, plan, b, n_images, d_tbl, want_labels, sets[k].clustering_eps,
                                       sets[k].clustering_min_pts, stream, nullptr);
        if (rc != IS_OK) return rc;
        if (!pairwise) c->last_unary_path = plan.unary_walk;
    }
    return IS_OK;
}

int is_compute_sweep(is_ctx* c, const float* d_joined, const int32_t* d_seg, const float* h_gf, const float* h_ng,
                     const float* h_is2, const int* h_vhor, int pairwise, int n_images, const is_sweep_set* h_sets,
                     int n_sets, is_section* d_sections, const is_instance_buffers* instances, void* stream_) {
    if (!h_sets) return fail_arg("null pointer");
    if (n_sets < 1) return fail_arg("n_sets < 1");
    if (!h_gf || !h_ng || !h_is2 || !h_vhor) return fail_arg("null pointer");
    if (const char* fault = compute_fault(c, d_joined, d_seg, n_images, d_sections,
                                          instances, (long long)n_sets * (n_images > 0 ? n_images : 0)))
        return fail_arg(fault);
    if ((long long)n_sets * n_images * c->dp.C * c->dp.S > 0x7fffffffLL)
        return fail_arg("n_sets * n_images * realcols * max_sections does not fit 31 bits");
    for (int k = 0; k < n_sets; k++)
        if (h_sets[k].reserved != 0) return fail_arg("is_sweep_set.reserved must be 0");
    if (((uintptr_t)d_sections) & 15) return fail_arg("d_sections must be 16-byte aligned");
    ON_CTX_DEVICE(c);
    hipStream_t stream = (hipStream_t)stream_;
    const int rc_res = sweep_reserve(c, (size_t)n_sets * n_images * c->dp.C, instances ? (size_t)n_sets * n_images : 0);
    if (rc_res != IS_OK) return rc_res;
    int slot = 0;
    const int rc_stage = stage_call(c, h_gf, h_ng, h_is2, h_vhor, n_images, nullptr, &slot);
    if (rc_stage != IS_OK) return rc_stage;
    const int rc = sweep_enqueue(c, d_joined, d_seg, pairwise, n_images, h_sets, n_sets, d_sections, instances, stream,
                                 slot);
    if (rc != IS_OK) clear_call_state(c, stream);
    return rc;
}

int is_recluster(is_ctx* c, const is_section* d_sections, int n_images, float eps, int min_pts, int size_filter,
                 const is_instance_buffers* instances, void* stream_) {
    if (!c || !d_sections || !instances) return fail_arg("null pointer");
    if (n_images < 1 || n_images > c->max_batch || n_images > 65535) return fail_arg("n_images outside [1, max_batch]");
    for (int i = 0; i < n_images; i++)
        if (!instances[i].d_indices || !instances[i].d_centerofmass || !instances[i].d_core_candidates ||
            !instances[i].d_instances_per_class || !instances[i].d_labels)
            return fail_arg("d_indices, d_centerofmass, d_core_candidates, d_instances_per_class and d_labels are "
                            "required for every image");
    ON_CTX_DEVICE(c);
    hipStream_t stream = (hipStream_t)stream_;
    const int rc_res = sweep_reserve(c, 0, (size_t)n_images);
    if (rc_res != IS_OK) return rc_res;
    const int rc_stage = sweep_stage_instances(c, instances, (size_t)n_images, stream);
    if (rc_stage != IS_OK) return rc_stage;
    const int n_slots = c->dp.C * c->dp.S;
    HIP_TRY(isk_launch_recore(n_slots, c->dp.S, size_filter, n_images, d_sections, c->d_sweep_inst, stream));
    HIP_TRY(isk_launch_cluster(n_slots, eps, min_pts, n_images, c->d_sweep_inst, nullptr, c->d_cluster_scratch,
                               stream));
    return IS_OK;
}
