// kb_censusframe.h — the host frame the seven censuses share (view, reciprocity, classes, latency, contact age, delta,
// islands; DESIGN.md "Host control plane"): argument and handle checks, the device-time figures, scratch that grows,
// the download into host vectors and the copy into the caller's arrays.  A census supplies its kernels, its *Part, its
// leaf overloads on kb_sim* / SpSim* and its summary; the rest is here, once.  Its other half: kb_bitpass.h (device)
// and kb_scratch.h (scratch carver, rows-per-wave plan).  Included by kb_sim.hip after kb_ctl.h, before both.
#pragma once

// the first pointer that is set (nullptr: the caller asked for none of these arrays)
template <class... P> static const void* any_of(const P*... p) {
  const void* r = nullptr;
  ((r = r ? r : static_cast<const void*>(p)), ...);
  return r;
}
// the summary is there, and an array that was asked for holds the capacity
static int census_caps(const char* who, const void* out, const void* ids_any, size_t cap_ids, size_t n_ids,
                       const void* rows_any, size_t cap_rows, size_t n_rows) {
  if (!out) return KB_INVALID_ARGUMENT;
  if ((ids_any && cap_ids < n_ids) || (rows_any && cap_rows < n_rows)) {
    seterr(std::string(who) + ": an output array is shorter than the capacity"); return KB_INVALID_ARGUMENT;
  }
  return KB_OK;
}
// The kinds of handle a census does not answer, each with the tail of its refusal (nullptr: answered).  Sparse rows
// are refused before a rank handle, a rank handle before dense rows.
struct Refuse { const char* rank; const char* sparse; const char* dense; };
static int census_gate(const kb_sim* s, const char* who, const Refuse& no) {
  const Kind kd = kind_of(s);
  std::string why;
  if (kd.sparse && no.sparse) why = std::string("sparse rows ") + no.sparse;
  else if (kd.rank && no.rank) why = std::string("a rank handle holds its own rows only") + no.rank + " (use kb_sim_create or kb_sim_create_local)";
  else if (!kd.sparse && no.dense) why = std::string("dense rows ") + no.dense;
  if (why.empty()) return KB_OK;
  seterr(std::string(who) + ": " + why);
  return KB_INVALID_OPERATION;
}

// device time of a span of a stream; a leaf adds it to its *Part, only the entry point writes kb_sim::census_ms
struct CsTimer {
  hipEvent_t a = nullptr, b = nullptr;
  bool start(hipStream_t st) { return hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, st) == hipSuccess; }
  void stop(hipStream_t st) { (void)hipEventRecord(b, st); }
  double ms() { float t = 0; if (a && b && hipEventElapsedTime(&t, a, b) != hipSuccess) t = 0; return t; }
  ~CsTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};
static int census_ms_get(kb_sim* s, CensusMs k, double* ms) {
  if (!s || !ms) return KB_INVALID_ARGUMENT;
  *ms = s->census_ms[k];
  return KB_OK;
}

// scratch of `bytes` that grows, never shrinks; the previous call has synchronised its stream, so nothing uses the
// old one.  `err` is the failure's text.
static int dev_reserve(void** buf, size_t* cap, size_t bytes, const char* err) {
  if (*buf && *cap >= bytes) return KB_OK;
  if (*buf) { (void)hipFree(*buf); *buf = nullptr; *cap = 0; }
  if (hipMalloc(buf, bytes) != hipSuccess) { *buf = nullptr; seterr(err); return KB_CAPACITY; }
  *cap = bytes;
  return KB_OK;
}
// what a *_of test surface works with: a device, a non-blocking stream of its own and one allocation; the stream is
// synchronised and everything released when the scope ends
struct OfScope {
  hipStream_t st = nullptr;
  void* buf = nullptr; size_t cap = 0;
  int open(int device, const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { seterr("no HIP device"); return KB_NO_DEVICE; }
    if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) { seterr(std::string(who) + ": no such device"); return KB_NO_DEVICE; }
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { st = nullptr; seterr(std::string(who) + ": stream"); return KB_IO_ERROR; }
    return KB_OK;
  }
  ~OfScope() {
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (buf) (void)hipFree(buf);
  }
};

// n elements at `dev` into v, on the stream (the caller synchronises)
template <class T> static hipError_t fetch(std::vector<T>& v, const void* dev, size_t n, hipStream_t st) {
  v.resize(n);
  return n ? hipMemcpyAsync(v.data(), dev, sizeof(T) * n, hipMemcpyDeviceToHost, st) : hipSuccess;
}
// into an array of the caller's, where it asked for it
template <class T> static void deliver(T* dst, const T* src, size_t n) { if (dst && n) memcpy(dst, src, sizeof(T) * n); }
template <class T> static void deliver(T* dst, const std::vector<T>& v) { deliver(dst, v.data(), v.size()); }
