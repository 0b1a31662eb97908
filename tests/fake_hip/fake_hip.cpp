// fake_hip.cpp - a double of the HIP runtime for the CPU sanitizer build of the library's device-facing host code
// (the Makefile's DEV_CPP - api.cpp, stages.cpp, transfer.cpp, comm.cpp, devxfer.cpp, frame.cpp - and the host halves of
// kernels*.hip; `make host-runtime-asan`).  It defines
// exactly the entry points those objects leave undefined.  "Device" memory is host heap, so the sanitizers see every copy
// or fill that overruns a buffer, every use after hipFree and every double free; kernels are never run: a launch is logged
// with its argument bytes, and every device pointer among them must be null or lie in a live allocation.  README.md says what
// is modelled and what is not; fake_hip.h has the controls.
#include "fake_hip.h"

#include <cxxabi.h>
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>

#include "kernels.hpp"

namespace {

struct Alloc {
  size_t size;
  long ordinal;
};
struct Graph {
  std::vector<FakeHipLaunch> nodes;
};
struct Stream {
  Graph* capture = nullptr;   // between hipStreamBeginCapture and hipStreamEndCapture
};
struct ParamType {
  std::string type;
  uint32_t size;
  std::vector<uint32_t> ptrs;   // offsets of the device pointers inside the parameter
};
struct Kernel {
  std::string mangled, name;
  bool sized = false, parsed = false;
  std::string unsized;          // the parameter type the double cannot size
  std::vector<ParamType> params;
};

// (the kernels register themselves from static constructors, possibly before this file's own: one function-local object)
struct State {
  std::map<uintptr_t, Alloc> allocs;
  size_t bytes = 0, heap_limit = 0;
  long next_ordinal = 0;
  std::set<void*> streams, events, graphs, execs, pinned;
  std::map<const void*, Kernel> kernels;
  std::vector<FakeHipLaunch> log;
  std::vector<std::string> violations;
  int armed_kind = -1;
  long armed_k = -1;
  bool fired = false, fired_capturing = false;
  const char* fired_at = "";
  long calls[FAKEHIP_NKINDS] = {0, 0, 0, 0};
  hipError_t last_error = hipSuccess;
  struct {
    dim3 grid, block;
    size_t lds;
    hipStream_t stream;
  } config[8];
  int nconfig = 0;
};
State& S() {
  static State* s = new State();   // never destroyed: __hipUnregisterFatBinary runs from static destructors
  return *s;
}

void violation(const std::string& what) {
  S().violations.push_back(what);
  std::fprintf(stderr, "fake_hip: %s\n", what.c_str());
}

// true: this call is the armed failure
bool inject(int kind, const char* who) {
  State& s = S();
  const long idx = s.calls[kind]++;
  if (s.armed_kind == kind && idx == s.armed_k) {
    s.armed_kind = -1;
    s.fired = true;
    s.fired_at = who;
    s.fired_capturing = false;
    for (void* p : s.streams) s.fired_capturing |= ((Stream*)p)->capture != nullptr;
    return true;
  }
  return false;
}

// ---- the parameters of a kernel, from its demangled signature ---------------------------------------------------------

// For each struct a kernel takes by value: its size (a changed struct is a compile error here) and its device pointers.
#define OFF(T, m) ((uint32_t)offsetof(T, m))
using sg::StageArgs;
void ptrs_StageArgs(std::vector<uint32_t>& o) {
  static_assert(sizeof(sg::StageArgs) == 600 && sizeof(sg::SrcStep) == 40, "StageArgs changed: revisit its pointer members here");
  for (uint32_t m : {OFF(StageArgs, in), OFF(StageArgs, out), OFF(StageArgs, aux), OFF(StageArgs, uabs), OFF(StageArgs, Dt), OFF(StageArgs, Lt),
                     OFF(StageArgs, md), OFF(StageArgs, mk), OFF(StageArgs, ftab), OFF(StageArgs, nbr_tab), OFF(StageArgs, fragV),
                     OFF(StageArgs, fragL), OFF(StageArgs, fragQ), OFF(StageArgs, dbg), OFF(StageArgs, sponge_slot), OFF(StageArgs, sponge_B),
                     OFF(StageArgs, sponge_sigma), OFF(StageArgs, sponge_pre), OFF(StageArgs, lam), OFF(StageArgs, mu), OFF(StageArgs, rho2),
                     OFF(StageArgs, item_list), OFF(StageArgs, src_slot), OFF(StageArgs, src_idx), OFF(StageArgs, src_vals)})
    o.push_back(m);
  for (int s = 0; s < 6; ++s) o.push_back(OFF(StageArgs, ghost) + 8u * s);
  o.push_back(OFF(StageArgs, src_step) + OFF(sg::SrcStep, ctr));
  o.push_back(OFF(StageArgs, src_step) + OFF(sg::SrcStep, weights));
}
void ptrs_T2Const(std::vector<uint32_t>&) { static_assert(sizeof(sg::T2Const) == 528, "T2Const changed: it held no pointer"); }
void ptrs_SrcStep(std::vector<uint32_t>& o) {
  static_assert(sizeof(sg::SrcStep) == 40, "SrcStep changed: revisit its pointer members here");
  o.push_back(OFF(sg::SrcStep, ctr));
  o.push_back(OFF(sg::SrcStep, weights));
}
void ptrs_RecvArgs(std::vector<uint32_t>& o) {
  static_assert(sizeof(sg::RecvArgs) == 96, "RecvArgs changed: revisit its pointer members here");
  for (uint32_t m : {OFF(sg::RecvArgs, ctr), OFF(sg::RecvArgs, item), OFF(sg::RecvArgs, lane), OFF(sg::RecvArgs, phi), OFF(sg::RecvArgs, trace)})
    o.push_back(m);
}
void ptrs_measure(std::vector<uint32_t>& o) {
  using A = sg::measure::Args;
  static_assert(sizeof(A) == 336, "measure::Args changed: revisit its pointer members here");
  for (uint32_t m : {OFF(A, ctr), OFF(A, Mtri), OFF(A, w), OFF(A, partial), OFF(A, out)}) o.push_back(m);
}
void ptrs_xcorr(std::vector<uint32_t>& o) {
  using A = sg::xcorr::Args;
  static_assert(sizeof(A) == 352, "xcorr::Args changed: revisit its pointer members here");
  for (uint32_t m : {OFF(A, ua), OFF(A, sa), OFF(A, ub), OFF(A, sb), OFF(A, M), OFF(A, acc)}) o.push_back(m);
}
void ptrs_inject(std::vector<uint32_t>& o) {
  using A = sg::inject::Args;
  static_assert(sizeof(A) == 104, "inject::Args changed: revisit its pointer members here");
  for (uint32_t m : {OFF(A, ctr), OFF(A, item), OFF(A, lane), OFF(A, start), OFF(A, psi), OFF(A, amp)}) o.push_back(m);
}
void ptrs_spectra(std::vector<uint32_t>& o) {
  using A = sg::spectra::Args;
  static_assert(sizeof(A) == 80, "spectra::Args changed: revisit its pointer members here");
  for (uint32_t m : {OFF(A, ctr), OFF(A, w), OFF(A, acc)}) o.push_back(m);
}
void ptrs_PackArgs(std::vector<uint32_t>& o) {
  static_assert(sizeof(sg::PackArgs) == 360, "PackArgs changed: revisit its pointer members here");
  for (int s = 0; s < 6; ++s) o.push_back(OFF(sg::PackArgs, out) + 8u * s);
}
#undef OFF
const struct {
  const char* name;
  uint32_t size;
  void (*ptrs)(std::vector<uint32_t>&);
} kStructs[] = {{"sg::StageArgs", sizeof(sg::StageArgs), ptrs_StageArgs},       {"sg::T2Const", sizeof(sg::T2Const), ptrs_T2Const},
                {"sg::SrcStep", sizeof(sg::SrcStep), ptrs_SrcStep},             {"sg::RecvArgs", sizeof(sg::RecvArgs), ptrs_RecvArgs},
                {"sg::measure::Args", sizeof(sg::measure::Args), ptrs_measure}, {"sg::xcorr::Args", sizeof(sg::xcorr::Args), ptrs_xcorr},
                {"sg::inject::Args", sizeof(sg::inject::Args), ptrs_inject},    {"sg::spectra::Args", sizeof(sg::spectra::Args), ptrs_spectra},
                {"sg::PackArgs", sizeof(sg::PackArgs), ptrs_PackArgs}};
const struct {
  const char* name;
  uint32_t size;
} kScalars[] = {{"int", 4},   {"unsigned int", 4}, {"long", 8}, {"unsigned long", 8},  {"long long", 8}, {"unsigned long long", 8},
                {"float", 4}, {"double", 8},       {"bool", 1}, {"char", 1},           {"short", 2}};

// a parameter's type without the blanks around it and without a top-level const
std::string trim(std::string t) {
  while (!t.empty() && t.front() == ' ') t.erase(t.begin());
  while (!t.empty() && t.back() == ' ') t.pop_back();
  if (t.compare(0, 6, "const ") == 0) t.erase(0, 6);
  if (t.size() >= 6 && t.compare(t.size() - 6, 6, " const") == 0) t.erase(t.size() - 6);
  return t;
}

void parse(Kernel& k) {
  k.parsed = true;
  const std::string& sig = k.name;
  const size_t close = sig.rfind(')');
  if (close == std::string::npos) {
    k.unsized = "(no parameter list)";
    return;
  }
  size_t open = close;
  for (int depth = 0; open > 0; --open) {
    if (sig[open] == ')') depth += 1;
    if (sig[open] == '(' && --depth == 0) break;
  }
  std::vector<std::string> types;
  std::string cur;
  int depth = 0;
  for (size_t i = open + 1; i < close; ++i) {
    const char c = sig[i];
    if (c == '<' || c == '(') depth += 1;
    if (c == '>' || c == ')') depth -= 1;
    if (c == ',' && depth == 0) {
      types.push_back(cur);
      cur.clear();
    } else {
      cur += c;
    }
  }
  if (!trim(cur).empty()) types.push_back(cur);
  for (const std::string& raw : types) {
    ParamType p;
    p.type = trim(raw);
    p.size = 0;
    if (!p.type.empty() && p.type.back() == '*') {
      p.size = 8;
      p.ptrs.push_back(0);
    }
    for (const auto& sc : kScalars)
      if (p.size == 0 && p.type == sc.name) p.size = sc.size;
    for (const auto& st : kStructs)
      if (p.size == 0 && p.type == st.name) {
        p.size = st.size;
        st.ptrs(p.ptrs);
      }
    if (p.size == 0) {
      k.unsized = p.type;
      return;
    }
    k.params.push_back(p);
  }
  k.sized = true;
}

// ---- launches, the audit, captures ------------------------------------------------------------------------------------

void resolve(FakeHipLaunch& e, const char* when) {
  State& s = S();
  for (FakeHipPtr& p : e.ptrs) {
    uintptr_t v;
    std::memcpy(&v, e.args.data() + p.at, 8);
    p.ordinal = -1;
    p.offset = p.size = 0;
    if (v == 0) continue;
    auto it = s.allocs.upper_bound(v);
    if (it != s.allocs.begin()) {
      --it;
      if (v < it->first + it->second.size) {
        p.ordinal = it->second.ordinal;
        p.offset = v - it->first;
        p.size = it->second.size;
        continue;
      }
    }
    p.ordinal = -2;
    char buf[96];
    std::snprintf(buf, sizeof(buf), ": argument byte %u holds %p, in no live allocation", p.at, (void*)v);
    violation(std::string("pointer audit, ") + when + ", " + e.name + buf);
  }
}

// a stream handed to the runtime: null (the legacy stream) or one that is alive
Stream* stream_of(hipStream_t st, const char* who) {
  if (!st) return nullptr;
  if (!S().streams.count((void*)st)) {
    violation(std::string(who) + ": a stream that is not alive");
    return nullptr;
  }
  return (Stream*)st;
}

// queue an entry on its stream: into the graph of a capture, else - kernels only - into the log
void queue(FakeHipLaunch&& e) {
  Stream* st = stream_of((hipStream_t)e.stream, e.name.c_str());
  resolve(e, st && st->capture ? "at capture" : "at launch");
  if (st && st->capture)
    st->capture->nodes.push_back(std::move(e));
  else if (e.op == 0)
    S().log.push_back(std::move(e));
}

// a host wait, or legacy-stream work, while a capture is open: the runtime refuses it, and it means a capture was left open
void no_open_capture(const char* who) {
  for (void* p : S().streams)
    if (((Stream*)p)->capture) {
      violation(std::string(who) + " while a stream is still capturing: a capture was never ended");
      return;
    }
}

FakeHipLaunch mem_entry(int op, const char* name, void* dst, const void* src, size_t n, hipStream_t stream) {
  FakeHipLaunch e;
  e.op = op;
  e.name = name;
  for (int i = 0; i < 3; ++i) e.grid[i] = e.block[i] = 1;
  e.lds = n;   // (the byte count of a fill or copy rides in this field)
  e.stream = (void*)stream;
  e.replay = false;
  e.args.resize(16);
  std::memcpy(e.args.data(), &dst, 8);
  std::memcpy(e.args.data() + 8, &src, 8);
  e.params = {{"void*", 0, 8}, {"void const*", 8, 8}};
  e.ptrs.push_back({0, -1, 0, 0});
  if (op == 2) e.ptrs.push_back({8, -1, 0, 0});
  return e;
}

}  // namespace

// ---- the controls (fake_hip.h) ----------------------------------------------------------------------------------------

extern "C" {

void fakehip_fail(int kind, long k) {
  State& s = S();
  for (long& c : s.calls) c = 0;
  s.fired = s.fired_capturing = false;
  s.fired_at = "";
  s.armed_kind = (k >= 0 && kind >= 0 && kind < FAKEHIP_NKINDS) ? kind : -1;
  s.armed_k = k;
}
long fakehip_calls(int kind) { return (kind >= 0 && kind < FAKEHIP_NKINDS) ? S().calls[kind] : -1; }
int fakehip_fired(void) { return S().fired ? 1 : 0; }
const char* fakehip_fired_at(void) { return S().fired_at; }
int fakehip_fired_capturing(void) { return S().fired_capturing ? 1 : 0; }
void fakehip_heap_limit(size_t bytes) { S().heap_limit = bytes; }
void fakehip_get_counts(fakehip_counts* out) {
  State& s = S();
  out->allocs = (long)s.allocs.size();
  out->bytes = s.bytes;
  out->streams = (long)s.streams.size();
  out->events = (long)s.events.size();
  out->graphs = (long)s.graphs.size();
  out->execs = (long)s.execs.size();
  out->pinned = (long)s.pinned.size();
  out->capturing = 0;
  for (void* p : s.streams) out->capturing += ((Stream*)p)->capture ? 1 : 0;
}
size_t fakehip_alloc_size(const void* p) {
  auto it = S().allocs.find((uintptr_t)p);
  return it == S().allocs.end() ? 0 : it->second.size;
}
size_t fakehip_violations(void) { return S().violations.size(); }
const char* fakehip_violation(size_t i) { return i < S().violations.size() ? S().violations[i].c_str() : ""; }
void fakehip_clear_violations(void) { S().violations.clear(); }

}  // extern "C"

const std::vector<FakeHipLaunch>& fakehip_log() { return S().log; }
void fakehip_log_clear() { S().log.clear(); }
std::vector<std::string> fakehip_kernels() {
  std::vector<std::string> out;
  for (const auto& kv : S().kernels) out.push_back(kv.second.name);
  return out;
}

// ---- the runtime's entry points ---------------------------------------------------------------------------------------

extern "C" {

// registration: what the host half of every kernels*.hip calls from its static constructor
void** __hipRegisterFatBinary(const void*) {
  static void* module = nullptr;
  return &module;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* hostFunction, char*, const char* deviceName, unsigned int, void*, void*, void*, void*, int*) {
  Kernel k;
  k.mangled = deviceName ? deviceName : "";
  int status = 0;
  char* d = abi::__cxa_demangle(k.mangled.c_str(), nullptr, nullptr, &status);
  k.name = (status == 0 && d) ? d : k.mangled;
  std::free(d);
  S().kernels[hostFunction] = k;
}
hipError_t __hipPushCallConfiguration(dim3 gridDim, dim3 blockDim, size_t sharedMem, hipStream_t stream) {
  State& s = S();
  if (s.nconfig >= 8) {
    violation("__hipPushCallConfiguration: eight launch configurations pushed and never popped");
    return s.last_error = hipErrorUnknown;
  }
  s.config[s.nconfig].grid = gridDim;
  s.config[s.nconfig].block = blockDim;
  s.config[s.nconfig].lds = sharedMem;
  s.config[s.nconfig].stream = stream;
  s.nconfig += 1;
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* gridDim, dim3* blockDim, size_t* sharedMem, hipStream_t* stream) {
  State& s = S();
  if (s.nconfig <= 0) {
    violation("__hipPopCallConfiguration without a pushed configuration");
    return hipErrorUnknown;
  }
  s.nconfig -= 1;
  *gridDim = s.config[s.nconfig].grid;
  *blockDim = s.config[s.nconfig].block;
  *sharedMem = s.config[s.nconfig].lds;
  *stream = s.config[s.nconfig].stream;
  return hipSuccess;
}

// the device: one MI355X
hipError_t hipGetDeviceCount(int* count) {
  *count = 1;
  return hipSuccess;
}
hipError_t hipSetDevice(int device) { return device == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* prop, int device) {
  if (device != 0) return hipErrorInvalidDevice;
  std::memset(prop, 0, sizeof(*prop));
  std::snprintf(prop->name, sizeof(prop->name), "fake MI355X");
  std::snprintf(prop->gcnArchName, sizeof(prop->gcnArchName), "gfx950");
  prop->multiProcessorCount = 256;
  prop->warpSize = 64;
  prop->maxThreadsPerBlock = 1024;
  prop->sharedMemPerBlock = 64 << 10;
  prop->maxSharedMemoryPerMultiProcessor = 160 << 10;
  prop->totalGlobalMem = (size_t)288 << 30;
  return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int* pi, hipDeviceAttribute_t attr, int device) {
  if (device != 0) return hipErrorInvalidDevice;
  switch (attr) {
    case hipDeviceAttributeMultiprocessorCount: *pi = 256; return hipSuccess;
    case hipDeviceAttributeWarpSize: *pi = 64; return hipSuccess;
    case hipDeviceAttributeMaxSharedMemoryPerMultiprocessor: *pi = 160 << 10; return hipSuccess;
    case hipDeviceAttributeMaxSharedMemoryPerBlock: *pi = 64 << 10; return hipSuccess;
    default: violation("hipDeviceGetAttribute: an attribute the double does not model"); return hipErrorInvalidValue;
  }
}
hipError_t hipDeviceGetStreamPriorityRange(int* leastPriority, int* greatestPriority) {
  *leastPriority = 1;
  *greatestPriority = -1;
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
  no_open_capture("hipDeviceSynchronize");
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorInvalidDevice: return "invalid device ordinal";
    case hipErrorUnknown: return "unknown error";
    default: return "error of the runtime double";
  }
}
hipError_t hipGetLastError(void) {
  const hipError_t e = S().last_error;
  S().last_error = hipSuccess;
  return e;
}

// memory
hipError_t hipMalloc(void** ptr, size_t size) {
  State& s = S();
  *ptr = nullptr;
  if (inject(FAKEHIP_ALLOC, "hipMalloc")) return hipErrorOutOfMemory;
  if (size > ((size_t)1 << 36) || (s.heap_limit && s.bytes + size > s.heap_limit)) return hipErrorOutOfMemory;
  void* p = std::malloc(size ? size : 1);
  if (!p) return hipErrorOutOfMemory;
  s.allocs[(uintptr_t)p] = Alloc{size, s.next_ordinal++};
  s.bytes += size;
  *ptr = p;
  return hipSuccess;
}
hipError_t hipFree(void* ptr) {
  State& s = S();
  if (!ptr) return hipSuccess;
  auto it = s.allocs.find((uintptr_t)ptr);
  if (it == s.allocs.end()) {
    violation("hipFree of a pointer that is no live allocation");
  } else {
    s.bytes -= it->second.size;
    s.allocs.erase(it);
  }
  std::free(ptr);   // (a double free is the sanitizer's to report)
  return hipSuccess;
}
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) {
  *ptr = nullptr;
  if (inject(FAKEHIP_ALLOC, "hipHostMalloc")) return hipErrorOutOfMemory;
  if (size > ((size_t)1 << 36)) return hipErrorOutOfMemory;
  void* p = std::malloc(size ? size : 1);
  if (!p) return hipErrorOutOfMemory;
  S().pinned.insert(p);
  *ptr = p;
  return hipSuccess;
}
hipError_t hipHostFree(void* ptr) {
  if (!ptr) return hipSuccess;
  if (!S().pinned.erase(ptr)) violation("hipHostFree of a pointer that is no live pinned buffer");
  std::free(ptr);
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t sizeBytes, hipMemcpyKind) {
  if (inject(FAKEHIP_COPY, "hipMemcpy")) return hipErrorUnknown;
  no_open_capture("hipMemcpy");
  std::memmove(dst, src, sizeBytes);
  return hipSuccess;
}
hipError_t hipMemset(void* dst, int value, size_t sizeBytes) {
  if (inject(FAKEHIP_COPY, "hipMemset")) return hipErrorUnknown;
  no_open_capture("hipMemset");
  std::memset(dst, value, sizeBytes);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t sizeBytes, hipMemcpyKind, hipStream_t stream) {
  if (inject(FAKEHIP_COPY, "hipMemcpyAsync")) return hipErrorUnknown;
  Stream* st = stream_of(stream, "hipMemcpyAsync");
  if (st && st->capture) {
    queue(mem_entry(2, "hipMemcpyAsync", dst, src, sizeBytes, stream));
    return hipSuccess;
  }
  std::memmove(dst, src, sizeBytes);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t sizeBytes, hipStream_t stream) {
  if (inject(FAKEHIP_COPY, "hipMemsetAsync")) return hipErrorUnknown;
  Stream* st = stream_of(stream, "hipMemsetAsync");
  if (st && st->capture) {
    queue(mem_entry(1, "hipMemsetAsync", dst, nullptr, sizeBytes, stream));
    return hipSuccess;
  }
  std::memset(dst, value, sizeBytes);
  return hipSuccess;
}

// streams and events
hipError_t hipStreamCreateWithPriority(hipStream_t* stream, unsigned int, int) {
  *stream = nullptr;
  if (inject(FAKEHIP_CREATE, "hipStreamCreateWithPriority")) return hipErrorUnknown;
  Stream* st = new Stream();
  S().streams.insert(st);
  *stream = (hipStream_t)st;
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) {
  Stream* st = stream_of(stream, "hipStreamDestroy");
  if (!st) return hipErrorInvalidValue;
  if (st->capture) violation("hipStreamDestroy of a stream that is still capturing");
  S().streams.erase(st);
  delete st;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
  Stream* st = stream_of(stream, "hipStreamSynchronize");
  if (st && st->capture) violation("hipStreamSynchronize on a stream that is still capturing: a capture was never ended");
  return hipSuccess;
}
static hipError_t event_create(hipEvent_t* event) {
  *event = nullptr;
  if (inject(FAKEHIP_CREATE, "hipEventCreate")) return hipErrorUnknown;
  void* e = std::malloc(8);
  S().events.insert(e);
  *event = (hipEvent_t)e;
  return hipSuccess;
}
static bool event_alive(hipEvent_t e, const char* who) {
  if (e && S().events.count((void*)e)) return true;
  violation(std::string(who) + ": an event that is not alive");
  return false;
}
hipError_t hipEventCreate(hipEvent_t* event) { return event_create(event); }
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned) { return event_create(event); }
hipError_t hipEventDestroy(hipEvent_t event) {
  if (!event_alive(event, "hipEventDestroy")) return hipErrorInvalidValue;
  S().events.erase((void*)event);
  std::free((void*)event);
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
  (void)stream_of(stream, "hipEventRecord");
  return event_alive(event, "hipEventRecord") ? hipSuccess : hipErrorInvalidValue;
}
hipError_t hipEventSynchronize(hipEvent_t event) {
  no_open_capture("hipEventSynchronize");
  return event_alive(event, "hipEventSynchronize") ? hipSuccess : hipErrorInvalidValue;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t start, hipEvent_t stop) {
  *ms = 0.0f;
  return (event_alive(start, "hipEventElapsedTime") && event_alive(stop, "hipEventElapsedTime")) ? hipSuccess : hipErrorInvalidValue;
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int) {
  (void)stream_of(stream, "hipStreamWaitEvent");
  return event_alive(event, "hipStreamWaitEvent") ? hipSuccess : hipErrorInvalidValue;
}

// captures and graphs.  A failed hipStreamEndCapture ends the capture all the same and hands back no graph, as the runtime's
// does (an invalidated capture); every other injected failure has no side effect.
hipError_t hipStreamBeginCapture(hipStream_t stream, hipStreamCaptureMode) {
  if (inject(FAKEHIP_CREATE, "hipStreamBeginCapture")) return hipErrorUnknown;
  Stream* st = stream_of(stream, "hipStreamBeginCapture");
  if (!st) return hipErrorInvalidValue;
  if (st->capture) {
    violation("hipStreamBeginCapture on a stream that is still capturing: a capture was never ended");
    return hipErrorInvalidValue;
  }
  st->capture = new Graph();
  S().graphs.insert(st->capture);
  return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t stream, hipGraph_t* pGraph) {
  *pGraph = nullptr;
  Stream* st = stream_of(stream, "hipStreamEndCapture");
  if (!st || !st->capture) return hipErrorInvalidValue;
  Graph* g = st->capture;
  st->capture = nullptr;
  if (inject(FAKEHIP_CREATE, "hipStreamEndCapture")) {
    S().graphs.erase(g);
    delete g;
    return hipErrorUnknown;
  }
  *pGraph = (hipGraph_t)g;
  return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t* pGraphExec, hipGraph_t graph, hipGraphNode_t*, char*, size_t) {
  *pGraphExec = nullptr;
  if (inject(FAKEHIP_CREATE, "hipGraphInstantiate")) return hipErrorUnknown;
  if (!S().graphs.count((void*)graph)) {
    violation("hipGraphInstantiate: a graph that is not alive");
    return hipErrorInvalidValue;
  }
  Graph* x = new Graph(*(Graph*)graph);
  S().execs.insert(x);
  *pGraphExec = (hipGraphExec_t)x;
  return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t graph) {
  if (!S().graphs.erase((void*)graph)) {
    violation("hipGraphDestroy: a graph that is not alive");
    return hipErrorInvalidValue;
  }
  delete (Graph*)graph;
  return hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t graphExec) {
  if (!S().execs.erase((void*)graphExec)) {
    violation("hipGraphExecDestroy: an executable graph that is not alive");
    return hipErrorInvalidValue;
  }
  delete (Graph*)graphExec;
  return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t graphExec, hipStream_t stream) {
  if (!S().execs.count((void*)graphExec)) {
    violation("hipGraphLaunch: an executable graph that is not alive");
    return hipErrorInvalidValue;
  }
  Stream* st = stream_of(stream, "hipGraphLaunch");
  if (st && st->capture) violation("hipGraphLaunch on a stream that is still capturing: a capture was never ended");
  // the frozen entries against the allocations that are live NOW
  for (const FakeHipLaunch& node : ((Graph*)graphExec)->nodes) {
    FakeHipLaunch e = node;
    e.replay = true;
    e.stream = (void*)stream;
    resolve(e, "at graph launch");
    if (e.op == 0) S().log.push_back(std::move(e));
  }
  return hipSuccess;
}

// kernels
hipError_t hipFuncSetAttribute(const void* func, hipFuncAttribute, int) {
  if (inject(FAKEHIP_LAUNCH, "hipFuncSetAttribute")) return hipErrorUnknown;
  if (!S().kernels.count(func)) violation("hipFuncSetAttribute: not a registered kernel");
  return hipSuccess;
}
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* numBlocks, const void* f, int, size_t) {
  if (inject(FAKEHIP_LAUNCH, "hipOccupancyMaxActiveBlocksPerMultiprocessor")) return hipErrorUnknown;
  if (!S().kernels.count(f)) violation("hipOccupancyMaxActiveBlocksPerMultiprocessor: not a registered kernel");
  *numBlocks = 2;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* function_address, dim3 numBlocks, dim3 dimBlocks, void** args, size_t sharedMemBytes,
                           hipStream_t stream) {
  State& s = S();
  if (inject(FAKEHIP_LAUNCH, "hipLaunchKernel")) return s.last_error = hipErrorUnknown;
  auto it = s.kernels.find(function_address);
  if (it == s.kernels.end()) {
    violation("hipLaunchKernel: not a registered kernel");
    return s.last_error = hipErrorInvalidDeviceFunction;
  }
  Kernel& k = it->second;
  if (!k.parsed) parse(k);
  if (!k.sized) {
    violation("hipLaunchKernel: cannot size parameter type '" + k.unsized + "' of " + k.name);
    return s.last_error = hipErrorInvalidValue;
  }
  if (numBlocks.x == 0 || numBlocks.y == 0 || numBlocks.z == 0 || dimBlocks.x * dimBlocks.y * dimBlocks.z == 0 ||
      dimBlocks.x * dimBlocks.y * dimBlocks.z > 1024) {
    violation("hipLaunchKernel: empty grid or a block the device does not take, " + k.name);
    return s.last_error = hipErrorInvalidConfiguration;
  }
  FakeHipLaunch e;
  e.op = 0;
  e.name = k.name;
  e.grid[0] = numBlocks.x, e.grid[1] = numBlocks.y, e.grid[2] = numBlocks.z;
  e.block[0] = dimBlocks.x, e.block[1] = dimBlocks.y, e.block[2] = dimBlocks.z;
  e.lds = sharedMemBytes;
  e.stream = (void*)stream;
  e.replay = false;
  for (size_t i = 0; i < k.params.size(); ++i) {
    const ParamType& p = k.params[i];
    const uint32_t at = (uint32_t)e.args.size();
    e.args.resize(at + p.size);
    std::memcpy(e.args.data() + at, args[i], p.size);
    e.params.push_back({p.type, at, p.size});
    for (uint32_t o : p.ptrs) e.ptrs.push_back({at + o, -1, 0, 0});
  }
  queue(std::move(e));
  return hipSuccess;
}

}  // extern "C"
