/* hip_shim.h — what the driver asks of the stand-in HIP runtime (hip_shim.cpp). */
#ifndef AMC_HIP_SHIM_H
#define AMC_HIP_SHIM_H

#ifdef __cplusplus
extern "C" {
#endif

/* the k-th device or pinned allocation from now fails with hipErrorOutOfMemory (that one alone); 0: none */
void shim_fail_alloc(long k);
/* 0 until the planned failure has happened, then the kind of the allocation that failed: 1 device, 2 pinned */
int shim_alloc_failed(void);
/* device and pinned allocations asked for / launches so far */
long shim_alloc_count(void);
long shim_launch_count(void);
/* device and pinned allocations, streams and events alive */
long shim_live_objects(void);
/* launches refused (a zero grid or block dimension, more than 1,024 threads per block), as "kernel grid block" lines */
long shim_bad_launch_count(void);
const char *shim_bad_launch(long k);
/* launches of kernels whose (demangled) name contains `part` */
long shim_launches_of(const char *part);

#ifdef __cplusplus
}
#endif
#endif
