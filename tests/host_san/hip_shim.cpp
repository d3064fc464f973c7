// hip_shim.cpp — a stand-in for the HIP runtime under the library's HOST code (tests/test_host_sanitized.py).
//
// The library's translation units are compiled host-only with AddressSanitizer and UBSan and linked against this file instead
// of libamdhip64: "device" and pinned memory are malloc blocks of exactly the size asked for, filled with 0xA5; copies and
// memsets act at once on those blocks, so an extent that runs past its allocation lands in ASan's red zone and a read-back of
// memory nobody cleared shows as 0xA5A5...; streams and events are one-byte blocks, so one that is never destroyed is a leak.
// A launch runs NOTHING: it is counted under the kernel's name and refused with hipErrorInvalidConfiguration when a grid or
// block dimension is zero or the block has more than 1,024 threads (the next hipGetLastError returns that error too).
// What this sees: host-enqueued extents, ownership, error paths, undefined read-backs, launch geometry.  Nothing a kernel does.
#include <cxxabi.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>
#include <hip/hip_ext.h>

#include "hip_shim.h"

namespace {

struct shim_state {
    std::map<const void *, std::string> kernels;     // host stub -> demangled kernel name
    std::map<std::string, long> launches_by_name;
    std::vector<std::string> bad;
    long allocs = 0, launches = 0, live = 0;
    long fail_in = 0;                                 // > 0: that many allocations from now, the last of them fails
    int failed = 0;
    hipError_t last = hipSuccess;
    bool verbose = false;
    // the open <<< >>> configuration
    dim3 grid, block;
    size_t shmem = 0;
    hipStream_t stream = nullptr;
};

// (the registration calls run from static constructors of the library's objects: built on first use, never destroyed)
shim_state &S()
{
    static shim_state *s = [] {
        shim_state *p = new shim_state;
        p->verbose = getenv("HIP_SHIM_VERBOSE") != nullptr;
        return p;
    }();
    return *s;
}

std::string demangle(const char *name)
{
    int status = 0;
    char *d = abi::__cxa_demangle(name, nullptr, nullptr, &status);
    std::string out = (status == 0 && d) ? d : name;
    free(d);
    // (templates' names come as "void k<...>(args)": the argument list says nothing here)
    const size_t par = out.rfind(")");
    if (par != std::string::npos) {
        int depth = 0;
        for (size_t k = par + 1; k-- > 0;) {
            if (out[k] == ')') depth++;
            else if (out[k] == '(' && --depth == 0) { out.erase(k); break; }
        }
    }
    return out;
}

hipError_t shim_alloc(void **p, size_t bytes, int kind)
{
    shim_state &s = S();
    if (!p) return hipErrorInvalidValue;
    s.allocs++;
    if (s.fail_in > 0 && --s.fail_in == 0) {
        s.failed = kind;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    void *q = malloc(bytes ? bytes : 1);
    if (!q) return hipErrorOutOfMemory;
    memset(q, 0xA5, bytes);
    s.live++;
    *p = q;
    return hipSuccess;
}

hipError_t shim_free(void *p)
{
    if (p) { S().live--; free(p); }
    return hipSuccess;
}

hipError_t shim_object(void **p)
{
    *p = malloc(1);
    if (!*p) return hipErrorOutOfMemory;
    S().live++;
    return hipSuccess;
}

hipError_t shim_launch(const void *f, dim3 g, dim3 b)
{
    shim_state &s = S();
    const auto it = s.kernels.find(f);
    const std::string name = it != s.kernels.end() ? it->second : "<a kernel that was never registered>";
    s.launches++;
    s.launches_by_name[name]++;
    char geom[160];
    snprintf(geom, sizeof geom, " grid (%u, %u, %u) block (%u, %u, %u)", g.x, g.y, g.z, b.x, b.y, b.z);
    if (s.verbose) fprintf(stderr, "[hip_shim] launch %s%s\n", name.c_str(), geom);
    const bool bad = !g.x || !g.y || !g.z || !b.x || !b.y || !b.z || (unsigned long long)b.x * b.y * b.z > 1024ULL ||
                     it == s.kernels.end();
    if (!bad) return hipSuccess;
    s.bad.push_back(name + geom);
    s.last = hipErrorInvalidConfiguration;
    return hipErrorInvalidConfiguration;
}

}  // namespace

// ---- the driver's controls ----------------------------------------------------------------------------------------------------
extern "C" {

void shim_fail_alloc(long k) { S().fail_in = k; S().failed = 0; }
int shim_alloc_failed(void) { return S().failed; }
long shim_alloc_count(void) { return S().allocs; }
long shim_launch_count(void) { return S().launches; }
long shim_live_objects(void) { return S().live; }
long shim_bad_launch_count(void) { return (long)S().bad.size(); }
const char *shim_bad_launch(long k) { return k >= 0 && k < (long)S().bad.size() ? S().bad[(size_t)k].c_str() : ""; }
long shim_launches_of(const char *part)
{
    long n = 0;
    for (const auto &kv : S().launches_by_name)
        if (kv.first.find(part) != std::string::npos) n += kv.second;
    return n;
}

// ---- the runtime ----------------------------------------------------------------------------------------------------------------
hipError_t hipGetDeviceCount(int *count) { *count = 1; return hipSuccess; }
hipError_t hipSetDevice(int device) { return device == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipDeviceGetAttribute(int *pi, hipDeviceAttribute_t attr, int device)
{
    if (!pi || device != 0) return hipErrorInvalidValue;
    *pi = attr == hipDeviceAttributeMultiprocessorCount ? 256 : 1;
    return hipSuccess;
}
hipError_t hipGetLastError(void)
{
    const hipError_t e = S().last;
    S().last = hipSuccess;
    return e;
}
const char *hipGetErrorString(hipError_t e)
{
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidConfiguration: return "invalid configuration argument";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorInvalidDevice: return "invalid device ordinal";
    default: return "an error the stand-in does not raise";
    }
}

hipError_t hipMalloc(void **p, size_t bytes) { return shim_alloc(p, bytes, 1); }
hipError_t hipFree(void *p) { return shim_free(p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return shim_alloc(p, bytes, 2); }
hipError_t hipHostFree(void *p) { return shim_free(p); }
hipError_t hipHostGetDevicePointer(void **dp, void *hp, unsigned int) { *dp = hp; return hipSuccess; }

hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t)
{
    if (bytes) memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t)
{
    if (bytes) memmove(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind)
{
    if (bytes) memmove(dst, src, bytes);
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { return shim_object((void **)s); }
hipError_t hipStreamDestroy(hipStream_t s) { return shim_free(s); }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
hipError_t hipStreamWriteValue32(hipStream_t, void *ptr, uint32_t value, unsigned int)
{
    memcpy(ptr, &value, sizeof value);      // (stored at once: nothing is in flight)
    return hipSuccess;
}
hipError_t hipStreamWaitValue32(hipStream_t, void *ptr, uint32_t, unsigned int, uint32_t)
{
    uint32_t v;
    memcpy(&v, ptr, sizeof v);              // (the word is read, so a bad address shows; nothing waits)
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int) { return shim_object((void **)e); }
hipError_t hipEventDestroy(hipEvent_t e) { return shim_free(e); }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }

// ---- launches and registration --------------------------------------------------------------------------------------------------
hipError_t hipLaunchKernel(const void *f, dim3 grid, dim3 block, void **, size_t, hipStream_t) { return shim_launch(f, grid, block); }
hipError_t hipExtLaunchKernel(const void *f, dim3 grid, dim3 block, void **, size_t, hipStream_t, hipEvent_t, hipEvent_t, int)
{
    return shim_launch(f, grid, block);
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream)
{
    shim_state &s = S();
    s.grid = grid; s.block = block; s.shmem = shmem; s.stream = stream;
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shmem, hipStream_t *stream)
{
    shim_state &s = S();
    *grid = s.grid; *block = s.block; *shmem = s.shmem; *stream = s.stream;
    return hipSuccess;
}
void **__hipRegisterFatBinary(const void *)
{
    static void *handle[1];
    return handle;
}
void __hipRegisterFunction(void **, const void *host_function, char *, const char *device_name, unsigned int, void *, void *, void *,
                           void *, int *)
{
    S().kernels[host_function] = demangle(device_name);
}
void __hipRegisterVar(void **, void *, char *, char *, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void **) {}

}  // extern "C"
