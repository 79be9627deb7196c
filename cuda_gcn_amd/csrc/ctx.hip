// ctx.hip — context: options, memory, graph capture, events.  The prepared adjacency and feature objects are
// graph.hip and feat.hip.
#include "common.h"
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ctype.h>

static thread_local char g_detail[256] = "";
int gcnhip_fail(const char *detail) {
    snprintf(g_detail, sizeof g_detail, "%s", detail ? detail : "");
    return -1;
}

const GcnOptionEntry GCN_OPTION_TABLE[] = {
    {"gs_u", &GcnOptions::gs_u, 0}, {"gs_l", &GcnOptions::gs_l, 0},
    {"gemm_bf16x3", &GcnOptions::gemm_bf16x3, 2}, {"spmm_slices", &GcnOptions::spmm_slices, 1},
    {"xent_finalize", &GcnOptions::xent_finalize, 0}, {"adam_sum_launch", &GcnOptions::adam_sum_launch, 0},
    {"spmm_rows", &GcnOptions::spmm_rows, 0}, {"spmm_general", &GcnOptions::spmm_general, 0}, {"spmm_nw", &GcnOptions::spmm_nw, 0}, {"split_edges", &GcnOptions::split_edges, 0},
};
const int GCN_OPTION_COUNT = (int)(sizeof GCN_OPTION_TABLE / sizeof GCN_OPTION_TABLE[0]);

// defaults, then GCNHIP_<NAME> from the environment (a set but empty or non-numeric variable means 1): once, here
static void options_from_environment(GcnOptions *o) {
    for (int i = 0; i < GCN_OPTION_COUNT; i++) {
        const GcnOptionEntry &e = GCN_OPTION_TABLE[i];
        o->*e.field = e.dflt;
        char var[64] = "GCNHIP_";
        size_t n = strlen(var);
        for (const char *q = e.name; *q && n + 1 < sizeof var; q++) var[n++] = (char)toupper((unsigned char)*q);
        var[n] = 0;
        if (const char *v = getenv(var)) {
            char *end;
            const long x = strtol(v, &end, 10);
            o->*e.field = end == v ? 1 : (int)x;
        }
    }
}

extern "C" {

const char *gcnhip_last_error(void) { return g_detail; }

int gcnhip_ctx_set_option(gcnhip_ctx *c, const char *name, int value) {
    if (!c || !name) return -1;
    for (int i = 0; i < GCN_OPTION_COUNT; i++)
        if (!strcmp(GCN_OPTION_TABLE[i].name, name)) { c->opt.*GCN_OPTION_TABLE[i].field = value; return 0; }
    return gcnhip_fail("gcnhip_ctx_set_option: unknown option");
}
int gcnhip_ctx_get_option(const gcnhip_ctx *c, const char *name, int *value) {
    if (!c || !name || !value) return -1;
    for (int i = 0; i < GCN_OPTION_COUNT; i++)
        if (!strcmp(GCN_OPTION_TABLE[i].name, name)) { *value = c->opt.*GCN_OPTION_TABLE[i].field; return 0; }
    return gcnhip_fail("gcnhip_ctx_get_option: unknown option");
}

int gcnhip_device_count(int *count) {
    GCNHIP_TRY(hipGetDeviceCount(count));
    return 0;
}

const char *gcnhip_error_string(int code) {
    if (code == -1) return "gcnhip: invalid argument";
    if (code == GCNHIP_NOT_AVAILABLE) return "gcnhip: this fused form is not available for these shapes / options (nothing was launched)";
    return hipGetErrorString((hipError_t)code);
}

const char *gcnhip_version(void) { return "gcnhip 0.1 (gfx950)"; }
int gcnhip_experiments(void) { return 0; }

int gcnhip_ctx_create(gcnhip_ctx **out, int device, void *stream) {
    if (!out) return -1;
    GCNHIP_TRY(hipSetDevice(device));
    std::unique_ptr<gcnhip_ctx, int (*)(gcnhip_ctx *)> c(new gcnhip_ctx(), gcnhip_ctx_destroy);
    c->device = device;
    options_from_environment(&c->opt);
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        GCNHIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    {   // code objects are loaded per device; gcn-hip's worker threads create their contexts at the same time
        static std::mutex mu;
        static bool preloaded[64] = {};
        std::lock_guard<std::mutex> lock(mu);
        if (device >= 0 && device < 64 && !preloaded[device]) {
            GCNHIP_TRY((hipError_t)gcnhip_preload_elementwise());
            GCNHIP_TRY((hipError_t)gcnhip_preload_graphsum());
            GCNHIP_TRY((hipError_t)gcnhip_preload_matmul());
            GCNHIP_TRY((hipError_t)gcnhip_preload_spmm());
            GCNHIP_TRY((hipError_t)gcnhip_preload_xent());
            GCNHIP_TRY((hipError_t)gcnhip_preload_bce());
            preloaded[device] = true;
        }
    }
    hipDeviceProp_t prop;
    GCNHIP_TRY(hipGetDeviceProperties(&prop, device));
    c->n_cu = prop.multiProcessorCount;
    GCNHIP_TRY(c->red_f.alloc(RED_SLOTS * 4));
    GCNHIP_TRY(c->red_i.alloc(RED_SLOTS * 4));
    GCNHIP_TRY(c->ticket.alloc(64));
    GCNHIP_TRY(hipMemset(c->ticket, 0, 64 * sizeof(uint32_t)));
    GCNHIP_TRY(c->wpack.alloc(WPACK_BYTES / sizeof(float)));
    c->wpack_bytes = WPACK_BYTES;
    *out = c.release();
    return 0;
}

int gcnhip_ctx_destroy(gcnhip_ctx *c) {
    if (!c) return 0;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

int gcnhip_ctx_set_corun(gcnhip_ctx *c, int on) {
    if (!c) return -1;
    c->corun = on ? 1 : 0;
    return 0;
}

int gcnhip_ctx_compute_units(const gcnhip_ctx *c, int *count) {
    if (!c || !count) return -1;
    *count = c->n_cu;
    return 0;
}

int gcnhip_ctx_sync(gcnhip_ctx *c) { GCNHIP_TRY(hipStreamSynchronize(c->stream)); return 0; }
void *gcnhip_ctx_stream(gcnhip_ctx *c) { return (void *)c->stream; }

int gcnhip_malloc(gcnhip_ctx *c, void **ptr, size_t bytes) {
    GCNHIP_TRY(hipSetDevice(c->device));
    GCNHIP_TRY(dev_malloc(ptr, bytes ? bytes : 16));
    return 0;
}
int gcnhip_free(gcnhip_ctx *c, void *ptr) {
    if (!ptr) return 0;
    GCNHIP_TRY(hipSetDevice(c->device));
    GCNHIP_TRY(dev_free(ptr));
    return 0;
}
int gcnhip_memset_async(gcnhip_ctx *c, void *ptr, int byte, size_t bytes) {
    if (bytes) GCNHIP_TRY(hipMemsetAsync(ptr, byte, bytes, c->stream));
    return 0;
}
int gcnhip_h2d(gcnhip_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes) GCNHIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    GCNHIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}
int gcnhip_d2h(gcnhip_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes) GCNHIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    GCNHIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}
int gcnhip_d2d_async(gcnhip_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes) GCNHIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int gcnhip_host_alloc(void **ptr, size_t bytes) {
    if (!ptr) return -1;
    GCNHIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 16, hipHostMallocDefault));
    return 0;
}
int gcnhip_host_free(void *ptr) {
    if (ptr) GCNHIP_TRY(hipHostFree(ptr));
    return 0;
}
int gcnhip_d2h_async(gcnhip_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c || !dst || !src) return -1;
    if (bytes) GCNHIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

int gcnhip_capture_begin(gcnhip_ctx *c) {
    GCNHIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    return 0;
}
int gcnhip_capture_end(gcnhip_ctx *c, void **graph_exec) {
    hipGraph_t graph = nullptr;
    GCNHIP_TRY(hipStreamEndCapture(c->stream, &graph));
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess) return (int)e;
    *graph_exec = (void *)exec;
    return 0;
}
int gcnhip_graph_launch(gcnhip_ctx *c, void *graph_exec) {
    GCNHIP_TRY(hipGraphLaunch((hipGraphExec_t)graph_exec, c->stream));
    return 0;
}
int gcnhip_graph_exec_destroy(void *graph_exec) {
    if (graph_exec) GCNHIP_TRY(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
    return 0;
}

int gcnhip_event_create(void **ev) { GCNHIP_TRY(hipEventCreate((hipEvent_t *)ev)); return 0; }
int gcnhip_event_create_sync(void **ev) { GCNHIP_TRY(hipEventCreateWithFlags((hipEvent_t *)ev, hipEventDisableTiming)); return 0; }
int gcnhip_event_destroy(void *ev) { GCNHIP_TRY(hipEventDestroy((hipEvent_t)ev)); return 0; }
int gcnhip_event_record(gcnhip_ctx *c, void *ev) { GCNHIP_TRY(hipEventRecord((hipEvent_t)ev, c->stream)); return 0; }
int gcnhip_stream_wait_event(gcnhip_ctx *c, void *ev) {
    GCNHIP_TRY(hipStreamWaitEvent(c->stream, (hipEvent_t)ev, 0));
    return 0;
}
int gcnhip_event_sync(void *ev) { GCNHIP_TRY(hipEventSynchronize((hipEvent_t)ev)); return 0; }
int gcnhip_event_elapsed_ms(void *start, void *stop, float *ms) {
    GCNHIP_TRY(hipEventSynchronize((hipEvent_t)stop));
    GCNHIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return 0;
}

}  // extern "C"
