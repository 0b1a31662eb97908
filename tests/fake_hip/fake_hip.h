/* fake_hip.h - the controls of the HIP runtime double (fake_hip.cpp, README.md): fault injection and the live counts as
 * plain C functions, the launch log and the registration table for C++ callers (tools/host_runtime_common.hpp and the
 * suites of host_runtime_driver over it). */
#ifndef SEIGEN_FAKE_HIP_H
#define SEIGEN_FAKE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the kinds of runtime calls a failure can be injected into */
enum fakehip_kind {
  FAKEHIP_ALLOC = 0,  /* hipMalloc, hipHostMalloc                                             -> hipErrorOutOfMemory */
  FAKEHIP_COPY = 1,   /* hipMemcpy, hipMemcpyAsync, hipMemset, hipMemsetAsync                 -> hipErrorUnknown */
  FAKEHIP_CREATE = 2, /* streams, events, hipGraphInstantiate, hipStreamBeginCapture / EndCapture -> hipErrorUnknown */
  FAKEHIP_LAUNCH = 3, /* hipLaunchKernel (also reported by the next hipGetLastError) and what is asked of the runtime about
                         a kernel: hipFuncSetAttribute, hipOccupancyMaxActiveBlocksPerMultiprocessor -> hipErrorUnknown */
  FAKEHIP_NKINDS = 4
};

/* Arm: the counts of all kinds restart at zero; the k-th call (0-based) of `kind` from now on returns its error and does
 * nothing else, then the injection disarms itself.  k < 0: count only. */
void fakehip_fail(int kind, long k);
long fakehip_calls(int kind);   /* calls of the kind since arming */
int fakehip_fired(void);        /* the armed failure has been returned ... */
const char* fakehip_fired_at(void);   /* ... by this entry point ("" before) */
int fakehip_fired_capturing(void);    /* ... while a stream was capturing */
/* hipMalloc beyond this many live device bytes returns hipErrorOutOfMemory (0: no limit).  Pinned buffers do not count;
 * hipMalloc and hipHostMalloc both refuse a single request above 2^36 bytes. */
void fakehip_heap_limit(size_t bytes);

typedef struct fakehip_counts {
  long allocs;     /* live hipMalloc allocations */
  size_t bytes;    /* ... and their bytes */
  long streams, events, graphs, execs, pinned;
  long capturing;  /* streams between hipStreamBeginCapture and hipStreamEndCapture */
} fakehip_counts;
void fakehip_get_counts(fakehip_counts* out);
/* bytes of the live allocation that STARTS at p, 0 if there is none */
size_t fakehip_alloc_size(const void* p);

/* what the double itself objects to: a device pointer of a launch outside every live allocation, a kernel whose
 * signature it cannot size, work on a stream whose capture was never ended, a host wait inside a capture, a handle of
 * the runtime used after its destruction */
size_t fakehip_violations(void);
const char* fakehip_violation(size_t i);
void fakehip_clear_violations(void);

#ifdef __cplusplus
}

#include <string>
#include <vector>

/* a device pointer among the argument bytes of a launch, resolved against the allocations live at the launch (or, for an
 * entry of a replayed graph, at the hipGraphLaunch) */
struct FakeHipPtr {
  uint32_t at;       /* offset of the 8 pointer bytes in FakeHipLaunch::args */
  long ordinal;      /* of the allocation (hipMalloc calls are numbered from 0), -1: a null pointer, -2: in no live allocation */
  size_t offset;     /* of the pointer in its allocation */
  size_t size;       /* of the allocation */
};
struct FakeHipParam {
  std::string type;  /* as the demangled signature spells it */
  uint32_t at, size; /* in FakeHipLaunch::args */
};
struct FakeHipLaunch {
  int op;            /* 0: kernel, 1: fill (hipMemsetAsync), 2: copy (hipMemcpyAsync) - 1 and 2 are logged inside captures only */
  std::string name;  /* the demangled signature, "void sg::mfma_stage_G<double, 4, 0, 1, 1>(sg::StageArgs)" */
  unsigned grid[3], block[3];
  size_t lds;
  void* stream;
  bool replay;       /* appended by hipGraphLaunch */
  std::vector<unsigned char> args;   /* the parameters' bytes one behind the other, in the order of the signature */
  std::vector<FakeHipParam> params;
  std::vector<FakeHipPtr> ptrs;
};
const std::vector<FakeHipLaunch>& fakehip_log();
void fakehip_log_clear();
/* the demangled signatures of every kernel the program registered (__hipRegisterFunction) */
std::vector<std::string> fakehip_kernels();
#endif

#endif
