// ref_driver -- runs the fitted code's own CPU-mode translation units (pdfz and the NLL kernels,
// compiled unmodified against the stand-in headers in shim/) on one case file and writes what
// they computed to one result file.  Test infrastructure only: tests/golden/make_reference_parity.py
// records its results, tests/test_reference_parity_cpu.py replays them.
//
//   ref_driver pdfz CASE RESULT
//   ref_driver nll  CASE RESULT
//
// Case and result files are lists of named arrays:
//   "SXRC" u32 count, then per array: u32 name length, name, u8 type, u64 elements, raw bytes
//   type: 0 = i32, 1 = u32, 2 = f32, 3 = f64, 4 = i16
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <TRandom.h>
#include <sxmc/nll_kernels.h>
#include <sxmc/pdfz.h>

// declared by the fitted code's utility header, defined in a translation unit this recipe does
// not compile; only the sampling member that the driver never calls uses it
unsigned nint(float) {
  std::fprintf(stderr, "ref_driver: nint() is not provided\n");
  std::abort();
}

namespace {

struct Blob {
  uint8_t type = 0;
  std::vector<unsigned char> bytes;
  template <typename T>
  T* as() { return reinterpret_cast<T*>(bytes.data()); }
  template <typename T>
  size_t count() const { return bytes.size() / sizeof(T); }
};

const size_t kTypeSize[] = {4, 4, 4, 8, 2};

[[noreturn]] void die(const std::string& msg) {
  std::fprintf(stderr, "ref_driver: %s\n", msg.c_str());
  std::exit(2);
}

typedef std::map<std::string, Blob> Case;

Case read_case(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) die(std::string("cannot open ") + path);
  char magic[4];
  uint32_t count = 0;
  if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "SXRC", 4) != 0) die("bad magic");
  if (std::fread(&count, 4, 1, f) != 1) die("truncated header");
  Case c;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t len = 0;
    if (std::fread(&len, 4, 1, f) != 1 || len > 256) die("bad name length");
    std::string name(len, '\0');
    if (len && std::fread(&name[0], 1, len, f) != len) die("truncated name");
    Blob b;
    uint64_t n = 0;
    if (std::fread(&b.type, 1, 1, f) != 1 || b.type > 4) die("bad type");
    if (std::fread(&n, 8, 1, f) != 1 || n > (1u << 26)) die("bad element count");
    b.bytes.resize(n * kTypeSize[b.type]);
    if (!b.bytes.empty() && std::fread(b.bytes.data(), 1, b.bytes.size(), f) != b.bytes.size()) {
      die("truncated array " + name);
    }
    c[name] = b;
  }
  std::fclose(f);
  return c;
}

struct Writer {
  FILE* f;
  uint32_t count = 0;
  explicit Writer(const char* path) : f(std::fopen(path, "wb")) {
    if (!f) die(std::string("cannot write ") + path);
    std::fwrite("SXRC", 1, 4, f);
    std::fwrite(&count, 4, 1, f);
  }
  void put(const std::string& name, uint8_t type, const void* data, uint64_t n) {
    uint32_t len = (uint32_t)name.size();
    std::fwrite(&len, 4, 1, f);
    std::fwrite(name.data(), 1, len, f);
    std::fwrite(&type, 1, 1, f);
    std::fwrite(&n, 8, 1, f);
    if (n) std::fwrite(data, kTypeSize[type], n, f);
    count++;
  }
  void close() {
    std::fseek(f, 4, SEEK_SET);
    std::fwrite(&count, 4, 1, f);
    if (std::fclose(f) != 0) die("write failed");
  }
};

Blob& need(Case& c, const std::string& name, uint8_t type) {
  Case::iterator it = c.find(name);
  if (it == c.end()) die("case has no array " + name);
  if (it->second.type != type) die("array " + name + " has the wrong type");
  return it->second;
}
int32_t* i32(Case& c, const char* n) { return need(c, n, 0).as<int32_t>(); }
uint32_t* u32(Case& c, const char* n) { return need(c, n, 1).as<uint32_t>(); }
float* f32(Case& c, const char* n) { return need(c, n, 2).as<float>(); }
double* f64(Case& c, const char* n) { return need(c, n, 3).as<double>(); }
int16_t* i16(Case& c, const char* n) { return need(c, n, 4).as<int16_t>(); }

template <typename T>
hemi::Array<T>* to_array(Blob& b) {
  size_t n = b.count<T>();
  hemi::Array<T>* a = new hemi::Array<T>(n, true);
  if (n) a->copyFromHost(b.as<T>(), n);
  return a;
}

// The evaluator's histogram and its table of read indices are protected members; a subclass may
// look at them without any change to the class.
struct OpenHist : public pdfz::EvalHist {
  using pdfz::EvalHist::EvalHist;
  hemi::Array<unsigned int>* Bins() { return this->bins; }
  hemi::Array<int>* ReadBins() { return this->read_bins; }
  int TotalBins() const { return this->total_nbins; }
  double BinVolume() const { return this->bin_volume; }
};

// meta (i32): nfields, nobs, dataset, param_offset, param_stride, out_offset, out_stride, norm_offset
// systs (i32): rows of (type, obs, extra_field, npars, p0, p1, p2)
int run_pdfz(Case& c, Writer& w) {
  const int32_t* meta = i32(c, "meta");
  if (need(c, "meta", 0).count<int32_t>() != 8) die("pdfz meta needs 8 entries");
  const int nfields = meta[0], nobs = meta[1];
  Blob& sb = need(c, "samples", 2);
  std::vector<float> samples(sb.as<float>(), sb.as<float>() + sb.count<float>());
  std::vector<double> lower(f64(c, "lower"), f64(c, "lower") + nobs);
  std::vector<double> upper(f64(c, "upper"), f64(c, "upper") + nobs);
  std::vector<int> nbins(i32(c, "nbins"), i32(c, "nbins") + nobs);
  Blob& pb = need(c, "points", 2);
  std::vector<float> points(pb.as<float>(), pb.as<float>() + pb.count<float>());

  hemi::Array<double>* params = to_array<double>(need(c, "params", 3));
  hemi::Array<float>* out = to_array<float>(need(c, "out", 2));
  hemi::Array<unsigned int>* norm = to_array<unsigned int>(need(c, "norm", 1));

  std::vector<hemi::Array<short>*> keep;
  try {
    OpenHist h(samples, nfields, nobs, lower, upper, nbins, (unsigned)meta[2], false);
    Blob& sy = need(c, "systs", 0);
    const int32_t* s = sy.as<int32_t>();
    for (size_t i = 0; i + 7 <= sy.count<int32_t>(); i += 7) {
      const int npars = s[i + 3];
      hemi::Array<short>* pars = new hemi::Array<short>(npars, true);
      for (int k = 0; k < npars; k++) pars->writeOnlyHostPtr()[k] = (short)s[i + 4 + k];
      keep.push_back(pars);
      switch (s[i]) {
        case pdfz::Systematic::SHIFT:
          h.AddSystematic(pdfz::ShiftSystematic(s[i + 1], pars));
          break;
        case pdfz::Systematic::SCALE:
          h.AddSystematic(pdfz::ScaleSystematic(s[i + 1], pars));
          break;
        case pdfz::Systematic::CTSCALE:
          h.AddSystematic(pdfz::CosThetaScaleSystematic(s[i + 1], pars));
          break;
        case pdfz::Systematic::RESOLUTION_SCALE:
          h.AddSystematic(pdfz::ResolutionScaleSystematic(s[i + 1], s[i + 2], pars));
          break;
        default:
          die("unknown systematic type");
      }
    }
    h.SetEvalPoints(points);
    h.SetParameterBuffer(params, meta[3], meta[4]);
    h.SetPDFValueBuffer(out, meta[5], meta[6]);
    h.SetNormalizationBuffer(norm, meta[7]);
    h.EvalAsync();
    h.EvalFinished();

    w.put("bins", 1, h.Bins()->readOnlyHostPtr(), h.Bins()->size());
    w.put("norm", 1, norm->readOnlyHostPtr(), norm->size());
    w.put("out", 2, out->readOnlyHostPtr(), out->size());
    w.put("read_bins", 0, h.ReadBins()->readOnlyHostPtr(), h.ReadBins()->size());
    int32_t total = h.TotalBins();
    double vol = h.BinVolume();
    w.put("total_nbins", 0, &total, 1);
    w.put("bin_volume", 3, &vol, 1);
  } catch (pdfz::Error& e) {
    die("pdfz::Error: " + e.msg);
  }
  for (size_t i = 0; i < keep.size(); i++) delete keep[i];
  delete params;
  delete out;
  delete norm;
  return 0;
}

void put_rng_log(Writer& w) {
  std::vector<int32_t> kind;
  std::vector<double> args;
  for (size_t i = 0; i < gRandom->log.size(); i++) {
    kind.push_back(gRandom->log[i].kind);
    args.push_back(gRandom->log[i].a);
    args.push_back(gRandom->log[i].b);
    args.push_back(gRandom->log[i].popped);
  }
  w.put("rng_kind", 0, kind.data(), kind.size());
  w.put("rng_args", 3, args.data(), args.size());
  int32_t left = (int32_t)gRandom->queue.size();
  w.put("rng_left", 0, &left, 1);
}

// meta (i32): op, then per op
//   0 chunks  : ne, ns
//   1 reduce  : n
//   2 total   : nparameters, nsignals, nsources
//   3 decider : nparameters
//   4 pick    : n
//   5 combo   : nparameters, nsignals, nsources, npartial, nsteps, debug
int run_nll(Case& c, Writer& w) {
  const int32_t* meta = i32(c, "meta");
  Case::iterator q = c.find("rng");
  if (q != c.end()) {
    for (size_t i = 0; i < q->second.count<double>(); i++) {
      gRandom->queue.push_back(q->second.as<double>()[i]);
    }
  }
  RNGState rng = 0;
  switch (meta[0]) {
    case 0: {
      Blob& sums = need(c, "sums", 3);
      HEMI_KERNEL_LAUNCH(nll_event_chunks, 1, 1, 0, 0, f32(c, "lut"), f64(c, "pars"),
                         (size_t)meta[1], (size_t)meta[2], f64(c, "nexpected"), u32(c, "n_mc"),
                         i16(c, "source_id"), u32(c, "norms"), sums.as<double>());
      w.put("sums", 3, sums.as<double>(), sums.count<double>());
      break;
    }
    case 1: {
      double total = 0;
      HEMI_KERNEL_LAUNCH(nll_event_reduce, 1, 1, 0, 0, (size_t)meta[1], f64(c, "sums"), &total);
      w.put("total", 3, &total, 1);
      break;
    }
    case 2: {
      Blob& nll = need(c, "nll", 3);
      HEMI_KERNEL_LAUNCH(nll_total, 1, 1, 0, 0, (size_t)meta[1], f64(c, "pars"), (size_t)meta[2],
                         (size_t)meta[3], f64(c, "means"), f64(c, "sigmas"),
                         f64(c, "events_total"), f64(c, "nexpected"), u32(c, "n_mc"),
                         i16(c, "source_id"), u32(c, "norms"), nll.as<double>());
      w.put("nll", 3, nll.as<double>(), nll.count<double>());
      break;
    }
    case 3: {
      Blob& jb = need(c, "jump_buffer", 2);
      Blob& vc = need(c, "v_current", 3);
      HEMI_KERNEL_LAUNCH(jump_decider, 1, 1, 0, 0, &rng, f64(c, "nll_current"),
                         f64(c, "nll_proposed"), vc.as<double>(), f64(c, "v_proposed"),
                         (unsigned)meta[1], i32(c, "accepted"), i32(c, "counter"),
                         jb.as<float>());
      w.put("nll_current", 3, f64(c, "nll_current"), 1);
      w.put("v_current", 3, vc.as<double>(), vc.count<double>());
      w.put("accepted", 0, i32(c, "accepted"), 1);
      w.put("counter", 0, i32(c, "counter"), 1);
      w.put("jump_buffer", 2, jb.as<float>(), jb.count<float>());
      break;
    }
    case 4: {
      Blob& vp = need(c, "v_proposed", 3);
      HEMI_KERNEL_LAUNCH(pick_new_vector, 1, 1, 0, 0, (int)meta[1], &rng, f32(c, "jump_width"),
                         f64(c, "v_current"), vp.as<double>());
      w.put("v_proposed", 3, vp.as<double>(), vp.count<double>());
      break;
    }
    case 5: {
      const int np = meta[1], npartial = meta[4], nsteps = meta[5];
      Blob& jb = need(c, "jump_buffer", 2);
      Blob& vc = need(c, "v_current", 3);
      Blob& vp = need(c, "v_proposed", 3);
      if (need(c, "sums", 3).count<double>() != (size_t)npartial * nsteps) die("combo sums size");
      std::vector<double> trace;   // per step: nll_current, nll_proposed, v_current, v_proposed
      std::vector<int32_t> itrace; // per step: accepted, counter, draws so far
      for (int s = 0; s < nsteps; s++) {
        HEMI_KERNEL_LAUNCH(finish_nll_jump_pick_combo, 1, 1, 0, 0, (size_t)npartial,
                           f64(c, "sums") + (size_t)s * npartial, (size_t)meta[2],
                           (size_t)meta[3], f64(c, "means"), f64(c, "sigmas"), &rng,
                           f64(c, "nll_current"), f64(c, "nll_proposed"), vc.as<double>(),
                           vp.as<double>(), i32(c, "accepted"), i32(c, "counter"),
                           jb.as<float>(), np, f32(c, "jump_width"), f64(c, "nexpected"),
                           u32(c, "n_mc"), i16(c, "source_id"), u32(c, "norms"), meta[6] != 0);
        trace.push_back(f64(c, "nll_current")[0]);
        trace.push_back(f64(c, "nll_proposed")[0]);
        trace.insert(trace.end(), vc.as<double>(), vc.as<double>() + np);
        trace.insert(trace.end(), vp.as<double>(), vp.as<double>() + np);
        itrace.push_back(i32(c, "accepted")[0]);
        itrace.push_back(i32(c, "counter")[0]);
        itrace.push_back((int32_t)gRandom->log.size());
      }
      w.put("trace", 3, trace.data(), trace.size());
      w.put("itrace", 0, itrace.data(), itrace.size());
      w.put("jump_buffer", 2, jb.as<float>(), jb.count<float>());
      break;
    }
    default:
      die("unknown nll op");
  }
  put_rng_log(w);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) die("usage: ref_driver pdfz|nll CASE RESULT");
  Case c = read_case(argv[2]);
  Writer w(argv[3]);
  int rc;
  if (std::strcmp(argv[1], "pdfz") == 0) {
    rc = run_pdfz(c, w);
  } else if (std::strcmp(argv[1], "nll") == 0) {
    rc = run_nll(c, w);
  } else {
    die("unknown mode");
  }
  w.close();
  return rc;
}
