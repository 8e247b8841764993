// The threads-and-streams contract of include/raymarcher_amd.h on real host threads (TEST INFRASTRUCTURE): "Calls on different
// streams or devices may be issued concurrently from different host threads; calls on ONE stream must come from one thread at a
// time".  A stand-alone host over the C ABI, the HIP runtime and std::thread — no Python, whose threads contend only by accident.
//
//   gpu_threads <case> <scenes dir> <out dir>        cases: frames entries field release counted timing light lattice
//
// A case is a set of FAMILIES, one per thread: a fixed sequence of ABI calls ("steps") over a set of output buffers, repeated for
// a number of rounds, every round into buffers of its own.  The serial pass makes every step alone, on the default stream, and
// keeps each buffer's bytes; it also dumps the whole frames it produced to <out dir> (NAME.scene: the tables, NAME.rgba: the
// pixels), which the Python test holds to the oracle; the cases light and lattice dump their inputs and every serial record
// (NAME.bin, the tables as NAME.tables), which the test holds to each entry's definition.  Then every thread creates its own non-
// blocking stream, waits at one barrier and makes its calls in a tight loop, with steady_clock stamps around each.  After the
// join and a device synchronise every buffer is read back: its guard bands (a poison word before and behind the payload) must be
// intact and its payload must equal the serial bytes.  `overlap` is the share of calls whose interval intersects a call of
// another thread (the wait for the device lock is inside the interval).  Process-wide switches are set once, before the barrier.
// One JSON line on stdout: {"case", "ok", "threads", "calls", "overlap", "first_mismatch", "wall_ms"}; exit status 0 iff ok, 3 where a
// HIP call failed or the library reported RM_ERR_DEVICE, 1 for any other mismatch.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "raymarcher_amd.h"

typedef std::vector<uint8_t> Bytes;
static const uint32_t kPoison = 0x7FA5A5A5u;  // a signalling NaN with a fixed payload: no kernel produces it
static const size_t kGuard = 4096;            // bytes of poison before and behind every payload

static std::string g_case, g_outDir;
static std::string g_firstMismatch;
static void mismatch(const std::string &what) { if (g_firstMismatch.empty()) g_firstMismatch = what; }
// a HIP call failed or the library reported RM_ERR_DEVICE: the exit status is 3, and the test starts no further process
static std::atomic<bool> g_deviceTrouble{false};

static std::string json_escape(const std::string &s) {
  std::string o;
  for (char c : s) {
    if (c == '"' || c == '\\') { o += '\\'; o += c; }
    else if ((unsigned char)c < 0x20) o += ' ';
    else o += c;
  }
  return o;
}
static int finish(int threads, int calls, double overlap, double wallMs) {
  const bool ok = g_firstMismatch.empty();
  std::printf("{\"case\": \"%s\", \"ok\": %s, \"threads\": %d, \"calls\": %d, \"overlap\": %.4f, \"first_mismatch\": %s%s%s, \"wall_ms\": %.3f}\n",
              g_case.c_str(), ok ? "true" : "false", threads, calls, overlap, ok ? "null" : "\"", ok ? "" : json_escape(g_firstMismatch).c_str(),
              ok ? "" : "\"", wallMs);
  std::fflush(stdout);
  return ok ? 0 : (g_deviceTrouble.load() ? 3 : 1);
}
// a failure of the set-up or of the serial pass: nothing was run on threads
static int give_up(const std::string &what) { mismatch(what); return finish(0, 0, 0.0, 0.0); }

#define HIP_TRY(expr)                                                                                        \
  do {                                                                                                       \
    const hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) { g_deviceTrouble = true; mismatch(std::string(#expr) + ": " + hipGetErrorString(e_)); return false; } \
  } while (0)

// ---------------------------------------------------------------------------------------------------- guarded device buffers
static size_t round256(size_t n) { return (n + 255) & ~size_t(255); }
struct Guarded {
  uint8_t *base = nullptr;
  size_t bytes = 0, total = 0;
  void *payload() const { return base + kGuard; }
};
static bool guarded_alloc(size_t bytes, Guarded *g) {
  g->bytes = bytes;
  g->total = kGuard + round256(bytes) + kGuard;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g->base), g->total));
  static std::vector<uint32_t> poison;
  if (poison.size() * 4 < g->total) poison.assign(g->total / 4 + 1, kPoison);
  HIP_TRY(hipMemcpy(g->base, poison.data(), g->total, hipMemcpyHostToDevice));
  return true;
}
// the whole allocation back on the host: the guards (and the padding up to 256 bytes) must hold the poison; → the payload
static bool guarded_read(const Guarded &g, const std::string &what, Bytes *payload) {
  Bytes all(g.total);
  HIP_TRY(hipMemcpy(all.data(), g.base, g.total, hipMemcpyDeviceToHost));
  const size_t lo = kGuard, hi = kGuard + g.bytes;
  for (size_t i = 0; i + 4 <= g.total; i += 4) {
    if (i + 4 > lo && i < hi) continue;  // a payload word (a word that straddles the payload's end is left out)
    uint32_t w;
    std::memcpy(&w, &all[i], 4);
    if (w != kPoison) {
      mismatch(what + ": guard band written, " + (i < lo ? std::to_string(lo - i) + " bytes before the payload" : std::to_string(i - hi) + " bytes past its end"));
      return false;
    }
  }
  payload->assign(all.begin() + (long)lo, all.begin() + (long)hi);
  return true;
}

// a read-only device input, prepared once
template <class T>
static bool upload(const std::vector<T> &v, T **out) {
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(out), v.size() * sizeof(T) + 256));
  HIP_TRY(hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return true;
}

// ---------------------------------------------------------------------------------------------------- scenes
struct SceneData {
  RmCamera cam{};
  std::vector<RmObject> objs;
  std::vector<RmLight> lights;
  RmGlobals g{};
  RmSettings s{};
  int W = 0, H = 0;
  int no() const { return (int)objs.size(); }
  int nl() const { return (int)lights.size(); }
};
static RmCameraData camera_data(float px, float py, float pz, float lx, float ly, float lz, float heightAngle) {
  RmCameraData cd;
  std::memset(&cd, 0, sizeof(cd));
  cd.pos[0] = px; cd.pos[1] = py; cd.pos[2] = pz; cd.pos[3] = 1.0f;
  cd.look[0] = lx; cd.look[1] = ly; cd.look[2] = lz;
  cd.up[1] = 1.0f;
  cd.heightAngle = heightAngle;
  return cd;
}
static bool scene_from_file(const std::string &path, int W, int H, SceneData *out) {
  RmScene *sc = nullptr;
  if (rm_scene_load(path.c_str(), &sc) != RM_OK) { mismatch("rm_scene_load " + path + ": " + rm_last_error()); return false; }
  RmCameraData cd;
  bool ok = rm_scene_camera_data(sc, &cd) == RM_OK && rm_camera_build(&cd, W, H, 0.1f, 100.0f, nullptr, nullptr, &out->cam) == RM_OK &&
            rm_scene_globals(sc, nullptr, &out->g) == RM_OK;
  if (ok) {
    out->objs.assign(rm_scene_objects(sc), rm_scene_objects(sc) + rm_scene_num_objects(sc));
    out->lights.assign(rm_scene_lights(sc), rm_scene_lights(sc) + rm_scene_num_lights(sc));
    rm_settings_default(&out->s);
    out->W = W; out->H = H;
  } else {
    mismatch("camera or globals of " + path + ": " + rm_last_error());
  }
  rm_scene_free(sc);
  return ok;
}
static RmObject primitive(int type, float tx, float ty, float tz, float sc, float r, float g, float b) {
  RmObject o;
  std::memset(&o, 0, sizeof(o));
  o.type = type;
  const float inv = 1.0f / sc;
  o.invModel[0] = o.invModel[5] = o.invModel[10] = inv;
  o.invModel[15] = 1.0f;
  o.invModel[12] = -tx * inv; o.invModel[13] = -ty * inv; o.invModel[14] = -tz * inv;
  o.scaleFactor = sc;
  o.shininess = 20.0f;
  o.ior = 1.3f;
  for (int i = 0; i < 3; i++) { o.cAmbient[i] = 0.1f; o.cSpecular[i] = 0.5f; }
  o.cDiffuse[0] = r; o.cDiffuse[1] = g; o.cDiffuse[2] = b;
  o.texLoc = -1;
  o.lightIdx = -1;
  return o;
}
static RmLight directional(float r, float g, float b, float dx, float dy, float dz) {
  RmLight l;
  std::memset(&l, 0, sizeof(l));
  l.type = RM_LIGHT_DIRECTIONAL;
  l.color[0] = r; l.color[1] = g; l.color[2] = b;
  l.dir[0] = dx; l.dir[1] = dy; l.dir[2] = dz;
  l.func[0] = 1.0f;
  return l;
}
static RmGlobals plain_globals() {
  RmGlobals g;
  std::memset(&g, 0, sizeof(g));
  g.ka = g.kd = g.ks = g.kt = 0.5f;
  g.power = 8.0f;
  return g;
}
// a sphere, a cube, a torus and a reflective floor slab under a directional and a point light: the plain table-walk class
static bool primitives_scene(int W, int H, SceneData *out) {
  out->objs = {primitive(RM_SPHERE, -1.25f, 0.0f, 0.0f, 1.0f, 0.8f, 0.3f, 0.2f), primitive(RM_CUBE, 1.25f, 0.0f, 0.25f, 1.0f, 0.2f, 0.4f, 0.9f),
               primitive(RM_TORUS, 0.0f, 1.0f, -0.5f, 2.0f, 0.3f, 0.9f, 0.3f), primitive(RM_CYLINDER, 0.0f, -1.0f, 0.5f, 0.5f, 0.9f, 0.8f, 0.4f)};
  out->lights = {directional(1.0f, 1.0f, 1.0f, -0.4f, -1.0f, -0.5f)};
  RmLight p;
  std::memset(&p, 0, sizeof(p));
  p.type = RM_LIGHT_POINT;
  p.color[0] = 0.8f; p.color[1] = 0.8f; p.color[2] = 1.0f;
  p.pos[0] = 3.0f; p.pos[1] = 4.0f; p.pos[2] = 4.0f;
  p.func[0] = 0.7f; p.func[1] = 0.04f;
  out->lights.push_back(p);
  out->g = plain_globals();
  rm_settings_default(&out->s);
  out->W = W; out->H = H;
  const RmCameraData cd = camera_data(0.0f, 0.5f, 6.0f, 0.0f, -0.1f, -1.0f, 0.7f);
  if (rm_camera_build(&cd, W, H, 0.1f, 100.0f, nullptr, nullptr, &out->cam) != RM_OK) { mismatch(std::string("rm_camera_build: ") + rm_last_error()); return false; }
  return true;
}
static bool bulb_scene(const std::string &scenes, int W, int H, SceneData *out) {
  if (!scene_from_file(scenes + "/simple/unit_mandelbulb.json", W, H, out)) return false;
  out->s.fractalIters = 8;
  out->s.maxSteps = 96;
  return true;
}
// the wavefront pipeline's picture: the sponge, reflective, two bounces
static bool menger_scene(const std::string &scenes, int W, int H, SceneData *out) {
  if (!scene_from_file(scenes + "/simple/unit_mengersponge.json", W, H, out)) return false;
  for (RmObject &o : out->objs) o.cReflective[0] = o.cReflective[1] = o.cReflective[2] = 0.4f;
  out->s.mengerLevels = 4;
  out->s.enableReflection = 1;
  out->s.numReflection = 2;
  return true;
}

// terrain, sea, clouds and the sky over a sphere: the layer kernels and the noise texture
static bool layers_scene(int W, int H, float iTime, SceneData *land) {
  land->objs = {primitive(RM_SPHERE, 0.0f, 701.0f, -4.0f, 2.0f, 0.8f, 0.3f, 0.2f)};
  land->objs[0].cReflective[0] = land->objs[0].cReflective[1] = land->objs[0].cReflective[2] = 0.6f;
  land->lights = {directional(1.0f, 1.0f, 1.0f, -0.4f, -1.0f, -0.3f)};
  land->g = plain_globals();
  land->g.iTime = iTime;
  rm_settings_default(&land->s);
  land->s.features = RM_FEAT_SKY_BACKGROUND | RM_FEAT_TERRAIN | RM_FEAT_CLOUD | RM_FEAT_SEA | RM_FEAT_PERLIN_BUMP;
  land->s.enableReflection = 1;
  land->W = W; land->H = H;
  const RmCameraData cd = camera_data(0.0f, 700.0f, 6.0f, 0.0f, -0.2f, -1.0f, 0.87f);
  if (rm_camera_build(&cd, land->W, land->H, 0.1f, 100.0f, nullptr, nullptr, &land->cam) != RM_OK) { mismatch(std::string("rm_camera_build: ") + rm_last_error()); return false; }
  return true;
}
static void noise_texture(std::vector<uint8_t> *noise) {
  noise->resize(256 * 256 * 4);
  uint32_t lcg = 12345u;
  for (size_t i = 0; i < noise->size(); i++) { lcg = lcg * 1664525u + 1013904223u; (*noise)[i] = (i % 4 == 3) ? 255 : (uint8_t)(lcg >> 24); }
}

// the dump the Python test holds to the oracle: the tables as the ABI structs' bytes, then the pixels.  `ext`: ".scene" for a frame
// that the test renders with the oracle as it is; another extension where the tables are the input of records checked otherwise
static bool dump_frame(const std::string &name, const SceneData &sc, const Bytes &rgba, const std::vector<uint8_t> *noise, const char *ext = ".scene") {
  const std::string base = g_outDir + "/" + g_case + "_" + name;
  FILE *f = std::fopen((base + ext).c_str(), "wb");
  if (!f) { mismatch("cannot write " + base + ext); return false; }
  const int32_t head[6] = {sc.W, sc.H, sc.no(), sc.nl(), noise ? 1 : 0, 0};
  std::fwrite(head, sizeof(head), 1, f);
  std::fwrite(&sc.cam, sizeof(sc.cam), 1, f);
  std::fwrite(&sc.g, sizeof(sc.g), 1, f);
  std::fwrite(&sc.s, sizeof(sc.s), 1, f);
  std::fwrite(sc.objs.data(), sizeof(RmObject), sc.objs.size(), f);
  std::fwrite(sc.lights.data(), sizeof(RmLight), sc.lights.size(), f);
  std::fclose(f);
  f = std::fopen((base + ".rgba").c_str(), "wb");
  if (!f) { mismatch("cannot write " + base + ".rgba"); return false; }
  std::fwrite(rgba.data(), 1, rgba.size(), f);
  std::fclose(f);
  if (noise) {
    f = std::fopen((base + ".noise").c_str(), "wb");
    if (!f) { mismatch("cannot write " + base + ".noise"); return false; }
    std::fwrite(noise->data(), 1, noise->size(), f);
    std::fclose(f);
  }
  return true;
}
// raw bytes of an input or of a serial record, for the Python test: <out dir>/<case>_NAME.bin
static bool dump_bytes(const std::string &name, const void *p, size_t n) {
  const std::string path = g_outDir + "/" + g_case + "_" + name + ".bin";
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) { mismatch("cannot write " + path); return false; }
  const bool ok = std::fwrite(p, 1, n, f) == n;
  std::fclose(f);
  if (!ok) mismatch("short write of " + path);
  return ok;
}
template <class T>
static bool dump_vector(const std::string &name, const std::vector<T> &v) { return dump_bytes(name, v.data(), v.size() * sizeof(T)); }
static bool dump_device(const std::string &name, const void *d, size_t n) {
  Bytes b(n);
  HIP_TRY(hipMemcpy(b.data(), d, n, hipMemcpyDeviceToHost));
  return dump_bytes(name, b.data(), n);
}

// ---------------------------------------------------------------------------------------------------- families
struct Ctx {
  void *const *buf;    // the round's buffers (payload pointers), in the family's order
  int variant;         // round % variants
  hipStream_t stream;  // NULL in the serial pass
  bool serial;
};
struct Step {
  std::string name;
  std::function<int(const Ctx &)> call;
  // serial pass only, after the step and a device synchronise: read a value back, assert the schedule (false: mismatch() was called)
  std::function<bool(const Ctx &)> afterSerial;
};
struct Family {
  std::string name;
  int rounds = 1, variants = 1;
  std::vector<size_t> bufBytes;
  std::vector<Step> steps;
  std::vector<std::vector<Bytes>> expect;  // [variant][buffer], from the serial pass
  // serial pass only, after a variant's buffers are read back: dump frames
  std::function<bool(int variant, const std::vector<Bytes> &)> dump;
};
static size_t frame_bytes(const SceneData &sc, int frames = 1) { return (size_t)frames * sc.W * sc.H * 16; }

static bool serial_pass(Family &fam) {
  fam.expect.assign((size_t)fam.variants, {});
  for (int v = 0; v < fam.variants; v++) {
    std::vector<Guarded> bufs(fam.bufBytes.size());
    std::vector<void *> ptrs;
    for (size_t b = 0; b < bufs.size(); b++) { if (!guarded_alloc(fam.bufBytes[b], &bufs[b])) return false; ptrs.push_back(bufs[b].payload()); }
    const Ctx ctx{ptrs.data(), v, nullptr, true};
    for (Step &st : fam.steps) {
      const int rc = st.call(ctx);
      if (rc == RM_ERR_DEVICE) g_deviceTrouble = true;
      if (rc != RM_OK) { mismatch("serial " + fam.name + "/" + st.name + ": status " + std::to_string(rc) + ": " + rm_last_error()); return false; }
      HIP_TRY(hipDeviceSynchronize());
      if (st.afterSerial && !st.afterSerial(ctx)) return false;
    }
    for (size_t b = 0; b < bufs.size(); b++) {
      Bytes p;
      if (!guarded_read(bufs[b], "serial " + fam.name + " buffer " + std::to_string(b), &p)) return false;
      fam.expect[(size_t)v].push_back(std::move(p));
      HIP_TRY(hipFree(bufs[b].base));
    }
    if (fam.dump && !fam.dump(v, fam.expect[(size_t)v])) return false;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------- threads
struct Stamp { int64_t t0, t1; };
struct Worker {
  Family *fam = nullptr;
  hipStream_t stream = nullptr;
  std::vector<std::vector<Guarded>> bufs;  // [round][buffer]
  std::vector<std::vector<void *>> ptrs;
  std::vector<Stamp> stamps;
  std::string error;
};
static int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct SpinBarrier {
  std::atomic<int> waiting{0};
  int n;
  explicit SpinBarrier(int n_) : n(n_) {}
  void wait() { waiting.fetch_add(1); while (waiting.load() < n) std::this_thread::yield(); }
};
static void run_worker(Worker *w, int tid, SpinBarrier *bar) {
  const hipError_t ce = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
  if (ce != hipSuccess) { g_deviceTrouble = true; w->error = std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(ce); }
  w->stamps.reserve((size_t)w->fam->rounds * w->fam->steps.size());
  bar->wait();
  if (!w->error.empty()) return;
  for (int r = 0; r < w->fam->rounds && w->error.empty(); r++) {
    const Ctx ctx{w->ptrs[(size_t)r].data(), r % w->fam->variants, w->stream, false};
    for (const Step &st : w->fam->steps) {
      const int64_t t0 = now_ns();
      const int rc = st.call(ctx);
      w->stamps.push_back({t0, now_ns()});
      if (rc == RM_ERR_DEVICE) g_deviceTrouble = true;
      if (rc != RM_OK) {
        w->error = "thread " + std::to_string(tid) + " " + w->fam->name + "/" + st.name + " round " + std::to_string(r) + ": status " + std::to_string(rc) + ": " + rm_last_error();
        break;
      }
    }
  }
  const hipError_t se = hipStreamSynchronize(w->stream);
  if (se != hipSuccess) g_deviceTrouble = true;
  if (se != hipSuccess && w->error.empty()) w->error = "thread " + std::to_string(tid) + " hipStreamSynchronize: " + hipGetErrorString(se);
}

// the families on one thread each → exit status
static int run_case(std::vector<Family> &fams, const std::function<bool()> &beforeThreads, const std::function<bool()> &afterJoin) {
  for (Family &f : fams) if (!serial_pass(f)) return finish(0, 0, 0.0, 0.0);
  const int n = (int)fams.size();
  std::vector<Worker> workers((size_t)n);
  for (int t = 0; t < n; t++) {
    Worker &w = workers[(size_t)t];
    w.fam = &fams[(size_t)t];
    w.bufs.assign((size_t)w.fam->rounds, std::vector<Guarded>(w.fam->bufBytes.size()));
    w.ptrs.assign((size_t)w.fam->rounds, {});
    for (int r = 0; r < w.fam->rounds; r++)
      for (size_t b = 0; b < w.fam->bufBytes.size(); b++) {
        if (!guarded_alloc(w.fam->bufBytes[b], &w.bufs[(size_t)r][b])) return finish(0, 0, 0.0, 0.0);
        w.ptrs[(size_t)r].push_back(w.bufs[(size_t)r][b].payload());
      }
  }
  if (hipDeviceSynchronize() != hipSuccess) { g_deviceTrouble = true; return give_up("hipDeviceSynchronize ahead of the threads failed"); }
  if (beforeThreads && !beforeThreads()) return finish(0, 0, 0.0, 0.0);
  SpinBarrier bar(n);
  std::vector<std::thread> threads;
  const int64_t w0 = now_ns();
  for (int t = 0; t < n; t++) threads.emplace_back(run_worker, &workers[(size_t)t], t, &bar);
  for (auto &t : threads) t.join();
  const double wallMs = (double)(now_ns() - w0) * 1e-6;
  int calls = 0, overlapped = 0;
  for (int a = 0; a < n; a++) {
    if (!workers[(size_t)a].error.empty()) mismatch(workers[(size_t)a].error);
    for (const Stamp &s : workers[(size_t)a].stamps) {
      calls++;
      bool hit = false;
      for (int b = 0; b < n && !hit; b++) {
        if (b == a) continue;
        for (const Stamp &o : workers[(size_t)b].stamps)
          if (o.t0 < s.t1 && s.t0 < o.t1) { hit = true; break; }
      }
      overlapped += hit ? 1 : 0;
    }
  }
  const double overlap = calls ? (double)overlapped / calls : 0.0;
  const hipError_t de = hipDeviceSynchronize();
  if (de != hipSuccess) { g_deviceTrouble = true; mismatch(std::string("hipDeviceSynchronize after the join: ") + hipGetErrorString(de)); return finish(n, calls, overlap, wallMs); }
  if (afterJoin && !afterJoin()) return finish(n, calls, overlap, wallMs);
  // every buffer of every round of every thread: guards intact, payload = the serial bytes
  for (int t = 0; t < n && g_firstMismatch.empty(); t++) {
    Worker &w = workers[(size_t)t];
    for (int r = 0; r < w.fam->rounds && g_firstMismatch.empty(); r++)
      for (size_t b = 0; b < w.fam->bufBytes.size(); b++) {
        const std::string what = "thread " + std::to_string(t) + " " + w.fam->name + " round " + std::to_string(r) + " buffer " + std::to_string(b);
        Bytes got;
        if (!guarded_read(w.bufs[(size_t)r][b], what, &got)) break;
        const Bytes &want = w.fam->expect[(size_t)(r % w.fam->variants)][b];
        if (got.size() != want.size() || std::memcmp(got.data(), want.data(), got.size()) != 0) {
          size_t at = 0;
          while (at < got.size() && at < want.size() && got[at] == want[at]) at++;
          mismatch(what + " differs from the serial result, first at byte " + std::to_string(at) + " of " + std::to_string(got.size()));
          break;
        }
      }
  }
  return finish(n, calls, overlap, wallMs);
}

// ---------------------------------------------------------------------------------------------------- step builders
static hipStream_t S(const Ctx &c) { return c.stream; }
static float *F(const Ctx &c, int b) { return static_cast<float *>(c.buf[b]); }

// rm_render of one picture into buffer 0, `rounds` times; path / split: what the serial pass asserts of the settled picture (0:
// nothing), after `settle` repeats of the serial call
static Family render_family(const std::string &name, const SceneData *sc, int rounds, const RmResources *res, int wantPath, bool wantSplit,
                            int settle, const std::vector<uint8_t> *noise) {
  Family f;
  f.name = name;
  f.rounds = rounds;
  f.bufBytes = {frame_bytes(*sc)};
  Step st;
  st.name = "rm_render_res";
  st.call = [sc, res, settle](const Ctx &c) {
    int rc = RM_OK;
    for (int k = 0; k < (c.serial ? settle : 1) && rc == RM_OK; k++)
      rc = rm_render_res(&sc->cam, sc->objs.data(), sc->no(), sc->lights.data(), sc->nl(), &sc->g, &sc->s, res, sc->W, sc->H, 0, sc->H, F(c, 0), nullptr, S(c));
    return rc;
  };
  st.afterSerial = [name, wantPath, wantSplit](const Ctx &) {
    if (wantPath && rm_debug_last_path() != wantPath) { mismatch(name + ": serial pass ran path " + std::to_string(rm_debug_last_path()) + ", the case is about path " + std::to_string(wantPath)); return false; }
    if (wantSplit && rm_debug_last_split() <= 0) { mismatch(name + ": the settled serial picture ran without the light split"); return false; }
    return true;
  };
  f.steps.push_back(st);
  f.dump = [name, sc, noise](int, const std::vector<Bytes> &e) { return dump_frame(name, *sc, e[0], noise); };
  return f;
}

// every buffer of a variant's serial pass as <case>_NAME_v<variant>_b<buffer>.bin
static std::function<bool(int, const std::vector<Bytes> &)> dump_buffers(const std::string &name) {
  return [name](int v, const std::vector<Bytes> &e) {
    for (size_t b = 0; b < e.size(); b++)
      if (!dump_vector(name + "_v" + std::to_string(v) + "_b" + std::to_string(b), e[b])) return false;
    return true;
  };
}

// "The tables, g, s … are host memory, copied before return": the host arguments of a step of the light case live in a scratch copy
// that the calling thread owns.  The thread fills it before the call and overwrites it with 0xFF bytes as soon as the call has
// returned — in the serial pass and on the threads alike —, so a library that read one of them later would read a table of NaNs.
struct HostArgs {
  std::vector<RmObject> objs;
  std::vector<RmLight> lights;
  RmGlobals g;
  RmSettings s;
  int dims[3];
  float origin[3], step[3];
  RmLightGridRef grid;
  int no() const { return (int)objs.size(); }
  int nl() const { return (int)lights.size(); }
  void spoil() {
    std::memset(static_cast<void *>(objs.data()), 0xFF, objs.size() * sizeof(RmObject));
    std::memset(static_cast<void *>(lights.data()), 0xFF, lights.size() * sizeof(RmLight));
    std::memset(static_cast<void *>(&g), 0xFF, sizeof(g));
    std::memset(static_cast<void *>(&s), 0xFF, sizeof(s));
    std::memset(dims, 0xFF, sizeof(dims));
    std::memset(origin, 0xFF, sizeof(origin));
    std::memset(step, 0xFF, sizeof(step));
    std::memset(static_cast<void *>(&grid), 0xFF, sizeof(grid));
  }
};
// the light case's probe grid: 5×4×3 probes over the box of the driver's points
static const int kGridDims[3] = {5, 4, 3};
static const float kGridOrigin[3] = {-2.75f, -2.25f, -2.25f}, kGridStep[3] = {1.375f, 1.5f, 2.25f};
static const float kLightFar = 100.0f, kDepthDistance = 8.0f, kNormalBias = 0.1f, kStrength = 0.8f;
// the lattice case's rm_field_ambient: origins a third of a step off the surface, rays as long as the lattice is deep
static const float kAmbBias = 0.1f, kAmbDistance = 2.0f;
static HostArgs &host_args(const SceneData &sc, const RmLightProbe *probes, const RmProbeDepth *depth, uint32_t flags) {
  thread_local HostArgs a;
  a.objs = sc.objs;
  a.lights = sc.lights;
  a.g = sc.g;
  a.s = sc.s;
  std::memcpy(a.dims, kGridDims, sizeof(a.dims));
  std::memcpy(a.origin, kGridOrigin, sizeof(a.origin));
  std::memcpy(a.step, kGridStep, sizeof(a.step));
  std::memset(&a.grid, 0, sizeof(a.grid));
  a.grid.d_probes = probes;
  a.grid.d_depth = depth;
  std::memcpy(a.grid.dims, kGridDims, sizeof(a.grid.dims));
  std::memcpy(a.grid.origin, kGridOrigin, sizeof(a.grid.origin));
  std::memcpy(a.grid.step, kGridStep, sizeof(a.grid.step));
  a.grid.strength = kStrength;
  a.grid.flags = flags;
  a.grid.normalBias = kNormalBias;
  return a;
}

int main(int argc, char **argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: gpu_threads <case> <scenes dir> <out dir>\n"); return 2; }
  g_case = argv[1];
  const std::string scenes = argv[2];
  g_outDir = argv[3];
  if (rm_set_device(0) != RM_OK) return give_up(std::string("rm_set_device: ") + rm_last_error());

  // ================================================================================================ frames
  if (g_case == "frames") {
    static SceneData bulb, lit, menger, land;
    if (!bulb_scene(scenes, 512, 264, &bulb) || !scene_from_file(scenes + "/lighting/directional_light_2.json", 512, 264, &lit) ||
        !menger_scene(scenes, 96, 61, &menger))
      return finish(0, 0, 0.0, 0.0);
    // soft shadows and AO, no secondary rays: the plain table-walk class, which the light split covers.  rm_set_kernel_path(5) is
    // process-wide and this picture is one the wavefront pipeline covers too, so more bounces than the pipeline takes (reflection
    // stays off: the count is not read by any pixel) keep it on the one-lane-per-pixel kernel, where the split lives.
    lit.s.enableSoftShadow = 1;
    lit.s.enableAmbientOcclusion = 1;
    lit.s.enableReflection = 0;
    lit.s.numReflection = 8;
    if (!layers_scene(72, 40, 0.7f, &land)) return finish(0, 0, 0.0, 0.0);
    static std::vector<uint8_t> noise;
    noise_texture(&noise);
    uint8_t *dNoise = nullptr;
    if (!upload(noise, &dNoise)) return finish(0, 0, 0.0, 0.0);
    static RmResources res;
    std::memset(&res, 0, sizeof(res));
    res.noise.pixels = dNoise; res.noise.width = 256; res.noise.height = 256;
    // the process-wide switches of the case, once, ahead of the serial pass and the threads alike
    if (rm_set_kernel_path(5) != RM_OK || rm_debug_set_light_split(1) != RM_OK) return give_up(std::string("switches: ") + rm_last_error());
    std::vector<Family> fams;
    fams.push_back(render_family("bulb", &bulb, 32, nullptr, 1, false, 1, nullptr));
    fams.push_back(render_family("light_split", &lit, 32, nullptr, 1, true, 20, nullptr));
    fams.push_back(render_family("wavefront", &menger, 32, nullptr, 5, false, 1, nullptr));
    fams.push_back(render_family("layers", &land, 32, &res, 1, false, 1, &noise));
    return run_case(fams, nullptr, nullptr);
  }

  // ================================================================================================ timing
  if (g_case == "timing") {
    static SceneData prim, bulb, menger, prim2;
    if (!primitives_scene(64, 40, &prim) || !bulb_scene(scenes, 64, 40, &bulb) || !menger_scene(scenes, 64, 40, &menger) || !primitives_scene(96, 61, &prim2))
      return finish(0, 0, 0.0, 0.0);
    std::vector<Family> fams;
    fams.push_back(render_family("primitives", &prim, 25, nullptr, 0, false, 1, nullptr));
    fams.push_back(render_family("bulb", &bulb, 25, nullptr, 0, false, 1, nullptr));
    fams.push_back(render_family("menger", &menger, 25, nullptr, 0, false, 1, nullptr));
    fams.push_back(render_family("primitives_96x61", &prim2, 25, nullptr, 0, false, 1, nullptr));
    const auto on = [] {
      double avg = 0.0;
      int launches = -1;
      // the switch goes on once, ahead of the barrier; the records of anything timed before are read and dropped
      if (rm_set_timing(1) != RM_OK || rm_get_timing(&avg, &launches) != RM_OK) { mismatch(std::string("rm_set_timing: ") + rm_last_error()); return false; }
      return true;
    };
    const auto off = [] {
      double avg = 0.0;
      int launches = -1;
      const int rc = rm_get_timing(&avg, &launches);
      const int rc2 = rm_set_timing(0);
      if (rc != RM_OK || rc2 != RM_OK) { mismatch(std::string("rm_get_timing: ") + rm_last_error()); return false; }
      if (launches != 100 || !(avg > 0.0)) { mismatch("rm_get_timing after 4 threads x 25 renders: launches " + std::to_string(launches) + ", average " + std::to_string(avg) + " ms"); return false; }
      return true;
    };
    return run_case(fams, on, off);
  }

  // ================================================================================================ counted
  if (g_case == "counted") {
    static SceneData prim, bulb, prod;
    if (!primitives_scene(64, 40, &prim) || !bulb_scene(scenes, 64, 40, &bulb) || !bulb_scene(scenes, 96, 61, &prod)) return finish(0, 0, 0.0, 0.0);
    const auto counted = [](const std::string &name, const SceneData *sc) {
      Family f;
      f.name = name;
      f.rounds = 10;
      f.bufBytes = {frame_bytes(*sc), frame_bytes(*sc), sizeof(RmCounters)};
      Step st;
      st.name = "rm_render_counted";
      st.call = [sc](const Ctx &c) {
        RmCounters n;
        std::memset(&n, 0, sizeof(n));
        const int rc = rm_render_counted(&sc->cam, sc->objs.data(), sc->no(), sc->lights.data(), sc->nl(), &sc->g, &sc->s, sc->W, sc->H, 0, sc->H, F(c, 0), F(c, 1), &n);
        if (rc != RM_OK) return rc;
        // the counters are a host result: they join the round's buffers so that they are compared like every other output
        return hipMemcpy(c.buf[2], &n, sizeof(n), hipMemcpyHostToDevice) == hipSuccess ? (int)RM_OK : (int)RM_ERR_DEVICE;
      };
      f.steps.push_back(st);
      f.dump = [name, sc](int, const std::vector<Bytes> &e) { return dump_frame(name, *sc, e[0], nullptr); };
      return f;
    };
    std::vector<Family> fams;
    fams.push_back(counted("counted_primitives", &prim));
    fams.push_back(counted("counted_bulb", &bulb));
    fams.push_back(render_family("production_bulb", &prod, 20, nullptr, 0, false, 1, nullptr));
    return run_case(fams, nullptr, nullptr);
  }

  // what entries, field and release share: the primitives, the bulb, rays, points
  static SceneData prim, bulb;
  if (!primitives_scene(64, 40, &prim) || !bulb_scene(scenes, 64, 40, &bulb)) return finish(0, 0, 0.0, 0.0);
  static const SceneData *two[2] = {&prim, &bulb};
  const int W = 64, H = 40, nRays = 4096;
  // 4096 rays: the primary rays of a 64×64 view of each scene
  static std::vector<RmRay> hostRays[2];
  static RmRay *dRays[2] = {nullptr, nullptr};
  for (int v = 0; v < 2; v++) {
    SceneData sq;
    if (!(v == 0 ? primitives_scene(64, 64, &sq) : bulb_scene(scenes, 64, 64, &sq))) return finish(0, 0, 0.0, 0.0);
    hostRays[v].resize((size_t)nRays);
    if (rm_camera_rays(&sq.cam, 64, 64, nullptr, nRays, hostRays[v].data()) != RM_OK) return give_up(std::string("rm_camera_rays: ") + rm_last_error());
    if (!upload(hostRays[v], &dRays[v])) return finish(0, 0, 0.0, 0.0);
  }
  // 4096 points on a jittered lattice through both scenes
  static std::vector<float> hostPoints((size_t)nRays * 4);
  {
    uint32_t lcg = 777u;
    const auto rnd = [&lcg] { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.0f / 16777216.0f); };
    for (int i = 0; i < nRays; i++) {
      hostPoints[(size_t)i * 4 + 0] = -2.75f + 5.5f * rnd();
      hostPoints[(size_t)i * 4 + 1] = -2.25f + 4.5f * rnd();
      hostPoints[(size_t)i * 4 + 2] = -2.25f + 4.5f * rnd();
      hostPoints[(size_t)i * 4 + 3] = 1.0f;
    }
  }
  static float *dPoints = nullptr;
  if (!upload(hostPoints, &dPoints)) return finish(0, 0, 0.0, 0.0);
  // 4096 unit normals, uniform over the sphere (light and lattice)
  static std::vector<float> hostNormals((size_t)nRays * 4);
  {
    uint32_t lcg = 4242u;
    const auto rnd = [&lcg] { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.0f / 16777216.0f); };
    for (int i = 0; i < nRays; i++) {
      const float z = 2.0f * rnd() - 1.0f, phi = 6.2831853f * rnd(), r = std::sqrt(std::fmax(0.0f, 1.0f - z * z));
      float n[3] = {r * std::cos(phi), r * std::sin(phi), z};
      const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      for (int a = 0; a < 3; a++) hostNormals[(size_t)i * 4 + a] = n[a] / len;
      hostNormals[(size_t)i * 4 + 3] = 0.0f;
    }
  }
  static float *dNormals = nullptr;
  if (!upload(hostNormals, &dNormals)) return finish(0, 0, 0.0, 0.0);
  // the 17×13×9 lattice and the 2×2×1 blocks (17×17×9 points) over the primitives
  static const float lo[3] = {-2.5f, -2.0f, -2.0f}, step[3] = {0.3125f, 1.0f / 3.0f, 0.5f};
  static const float blo[3] = {-2.5f, -2.5f, -2.0f}, bstep[3] = {0.3125f, 0.3125f, 0.5f};
  const int nx = 17, ny = 13, nz = 9, mx = 2, my = 2, mz = 1, maxBlocks = mx * my * mz;
  const int cells = (nx - 1) * (ny - 1) * (nz - 1), points = nx * ny * nz;
  static const float isoOf[2] = {0.0f, 0.001f};

  // ================================================================================================ entries
  if (g_case == "entries") {
    // three cameras a step apart, a thin lens of three samples, three object tables a step apart: per scene
    static std::vector<RmCamera> cams3[2], lens3[2];
    static std::vector<RmObject> tables3[2];
    for (int v = 0; v < 2; v++) {
      for (int k = 0; k < 3; k++) {
        const RmCameraData cd = camera_data(0.25f * (float)k, 0.5f, v == 0 ? 6.0f : 4.5f, -0.04f * (float)k, -0.1f, -1.0f, v == 0 ? 0.7f : 0.52f);
        RmCamera c;
        if (rm_camera_build(&cd, W, H, 0.1f, 100.0f, nullptr, nullptr, &c) != RM_OK) return give_up(std::string("rm_camera_build: ") + rm_last_error());
        cams3[v].push_back(c);
        const float move[3] = {0.125f * (float)k, 0.0f, -0.0625f * (float)k};
        for (const RmObject &o : two[v]->objs) {
          RmObject m;
          if (rm_object_translated(&o, move, &m) != RM_OK) return give_up(std::string("rm_object_translated: ") + rm_last_error());
          tables3[v].push_back(m);
        }
      }
      lens3[v].resize(3);
      const RmCameraData cd = camera_data(0.0f, 0.5f, v == 0 ? 6.0f : 4.5f, 0.0f, -0.1f, -1.0f, v == 0 ? 0.7f : 0.52f);
      if (rm_camera_lens_samples(&cd, W, H, 0.1f, 100.0f, 0.08f, 5.0f, 3, lens3[v].data()) != RM_OK) return give_up(std::string("rm_camera_lens_samples: ") + rm_last_error());
    }
    const size_t fb = (size_t)W * H * 16;
    std::vector<Family> fams;
    {
      Family f; f.name = "batch"; f.rounds = 24; f.variants = 2; f.bufBytes = {3 * fb, 3 * fb};
      f.steps.push_back({"rm_render_batch", [](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_render_batch(cams3[c.variant].data(), &s.g, 1, 3, s.objs.data(), s.no(), s.lights.data(), s.nl(), &s.s, nullptr, s.W, s.H, F(c, 0), F(c, 1), S(c)); }, nullptr});
      fams.push_back(f);
    }
    {
      Family f; f.name = "supersampled"; f.rounds = 24; f.variants = 2; f.bufBytes = {fb, fb};
      f.steps.push_back({"rm_render_supersampled", [](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_render_supersampled(&s.cam, &s.g, 1, 1, s.objs.data(), s.no(), s.lights.data(), s.nl(), &s.s, nullptr, s.W, s.H, 2, F(c, 0), F(c, 1), S(c)); }, nullptr});
      fams.push_back(f);
    }
    {
      Family f; f.name = "adaptive"; f.rounds = 24; f.variants = 2; f.bufBytes = {2 * fb, 2 * fb, (size_t)2 * W * H, 2 * sizeof(uint32_t)};
      f.steps.push_back({"rm_render_adaptive", [](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_render_adaptive(cams3[c.variant].data(), &s.g, 1, 2, s.objs.data(), s.no(), s.lights.data(), s.nl(), &s.s, nullptr, s.W, s.H, 2, 0.05f, F(c, 0), F(c, 1),
                                  static_cast<uint8_t *>(c.buf[2]), static_cast<uint32_t *>(c.buf[3]), S(c)); }, nullptr});
      fams.push_back(f);
    }
    {
      Family f; f.name = "accumulated_animated"; f.rounds = 12; f.variants = 2; f.bufBytes = {fb, fb, fb, fb};
      f.steps.push_back({"rm_render_accumulated", [](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_render_accumulated(lens3[c.variant].data(), &s.g, 1, 1, 3, s.objs.data(), s.no(), s.lights.data(), s.nl(), &s.s, nullptr, s.W, s.H, F(c, 0), F(c, 1), S(c)); }, nullptr});
      f.steps.push_back({"rm_render_animated", [](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_render_animated(cams3[c.variant].data(), &s.g, 1, tables3[c.variant].data(), s.no(), 3, s.lights.data(), s.nl(), 1, 1, 3, &s.s, nullptr, s.W, s.H, F(c, 2), F(c, 3), S(c)); }, nullptr});
      fams.push_back(f);
    }
    {
      Family f; f.name = "gbuffer"; f.rounds = 24; f.variants = 2; f.bufBytes = {2 * fb, (size_t)2 * W * H * 4, 2 * fb};
      f.steps.push_back({"rm_render_gbuffer", [](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_render_gbuffer(cams3[c.variant].data(), &s.g, 1, 2, s.objs.data(), s.no(), &s.s, s.W, s.H, F(c, 0), static_cast<int32_t *>(c.buf[1]), F(c, 2), S(c)); }, nullptr});
      fams.push_back(f);
    }
    {
      Family f; f.name = "rays_points"; f.rounds = 8; f.variants = 2;
      f.bufBytes = {(size_t)nRays * 32, (size_t)nRays * 16, (size_t)nRays * 16, (size_t)nRays * 32, (size_t)nRays * 4, (size_t)nRays * 16};
      f.steps.push_back({"rm_trace_rays", [nRays](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_trace_rays(dRays[c.variant], nRays, s.objs.data(), s.no(), &s.g, &s.s, RM_TRACE_CLOSEST, static_cast<RmRayHit *>(c.buf[0]), S(c)); }, nullptr});
      f.steps.push_back({"rm_shade_rays", [nRays](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_shade_rays(dRays[c.variant], nRays, 100.0f, s.objs.data(), s.no(), s.lights.data(), s.nl(), &s.g, &s.s, nullptr, F(c, 1), F(c, 2), S(c)); }, nullptr});
      f.steps.push_back({"rm_shade_points", [nRays](const Ctx &c) { const SceneData &s = *two[c.variant];
        RmPointsSettings ps;
        rm_points_settings_default(&ps);
        ps.projectSteps = 2;
        return rm_shade_points(dPoints, nullptr, nRays, &ps, s.objs.data(), s.no(), s.lights.data(), s.nl(), &s.g, &s.s, nullptr, static_cast<RmSurfacePoint *>(c.buf[3]), F(c, 4),
                               F(c, 5), S(c)); }, nullptr});
      fams.push_back(f);
    }
    static int nBlocks[2] = {0, 0};
    {
      Family f; f.name = "sdf"; f.rounds = 5; f.variants = 2;
      f.bufBytes = {(size_t)points * 4, (size_t)points * 4,                                                      // 0 dist, 1 ids
                    (size_t)cells * 16, (size_t)cells * 4, (size_t)points * 3 * 16, 2 * sizeof(uint32_t),       // 2 vertices, 3 vertex objects, 4 quads, 5 counts
                    (size_t)maxBlocks * 16, sizeof(uint32_t),                                                    // 6 blocks, 7 count
                    (size_t)maxBlocks * 729 * 4, (size_t)maxBlocks * 729 * 4,                                    // 8 block dist, 9 block ids
                    (size_t)maxBlocks * 512 * 16, (size_t)maxBlocks * 512 * 4, (size_t)maxBlocks * 512 * 3 * 16, 3 * sizeof(uint32_t)};  // 10-13
      f.steps.push_back({"rm_sdf_grid", [=](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_sdf_grid(s.objs.data(), s.no(), &s.g, &s.s, lo, step, nx, ny, nz, F(c, 0), static_cast<int32_t *>(c.buf[1]), S(c)); }, nullptr});
      f.steps.push_back({"rm_sdf_mesh", [=](const Ctx &c) {
        return rm_sdf_mesh(F(c, 0), static_cast<int32_t *>(c.buf[1]), nx, ny, nz, lo, step, isoOf[c.variant], cells, points * 3, F(c, 2), static_cast<int32_t *>(c.buf[3]),
                           static_cast<int32_t *>(c.buf[4]), static_cast<uint32_t *>(c.buf[5]), S(c)); }, nullptr});
      f.steps.push_back({"rm_sdf_blocks_select", [=](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_sdf_blocks_select(s.objs.data(), s.no(), &s.g, &s.s, blo, bstep, mx, my, mz, isoOf[c.variant], maxBlocks, static_cast<int32_t *>(c.buf[6]),
                                    static_cast<uint32_t *>(c.buf[7]), S(c)); },
        [=](const Ctx &c) {  // the list's length goes to the host once, alone; the threads pass it as a constant
          uint32_t n = 0;
          HIP_TRY(hipMemcpy(&n, c.buf[7], 4, hipMemcpyDeviceToHost));
          if (n > (uint32_t)maxBlocks) { mismatch("rm_sdf_blocks_select listed " + std::to_string(n) + " blocks of " + std::to_string(maxBlocks)); return false; }
          nBlocks[c.variant] = (int)n;
          return true;
        }});
      f.steps.push_back({"rm_sdf_grid_blocks", [=](const Ctx &c) { const SceneData &s = *two[c.variant];
        return rm_sdf_grid_blocks(s.objs.data(), s.no(), &s.g, &s.s, blo, bstep, mx, my, mz, static_cast<int32_t *>(c.buf[6]), nBlocks[c.variant], F(c, 8),
                                  static_cast<int32_t *>(c.buf[9]), S(c)); }, nullptr});
      f.steps.push_back({"rm_sdf_mesh_blocks", [=](const Ctx &c) {
        return rm_sdf_mesh_blocks(F(c, 8), static_cast<int32_t *>(c.buf[9]), static_cast<int32_t *>(c.buf[6]), nBlocks[c.variant], mx, my, mz, blo, bstep, isoOf[c.variant],
                                  maxBlocks * 512, maxBlocks * 512 * 3, F(c, 10), static_cast<int32_t *>(c.buf[11]), static_cast<int32_t *>(c.buf[12]),
                                  static_cast<uint32_t *>(c.buf[13]), S(c)); }, nullptr});
      fams.push_back(f);
    }
    {
      // inputs of the post passes and of rm_rays_restore, made alone: a frame with its BrightColor, the hits of the rays
      static float *dFrag = nullptr, *dBright = nullptr;
      static RmRayHit *dHits = nullptr;
      if (hipMalloc(reinterpret_cast<void **>(&dFrag), fb) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&dBright), fb) != hipSuccess ||
          hipMalloc(reinterpret_cast<void **>(&dHits), (size_t)nRays * 32) != hipSuccess)
        return give_up("hipMalloc of the post inputs failed");
      if (rm_render(&prim.cam, prim.objs.data(), prim.no(), prim.lights.data(), prim.nl(), &prim.g, &prim.s, W, H, 0, H, dFrag, dBright, nullptr) != RM_OK ||
          rm_trace_rays(dRays[0], nRays, prim.objs.data(), prim.no(), &prim.g, &prim.s, RM_TRACE_CLOSEST, dHits, nullptr) != RM_OK || hipDeviceSynchronize() != hipSuccess)
        return give_up(std::string("post inputs: ") + rm_last_error());
      Family f; f.name = "post_order"; f.rounds = 6;
      f.bufBytes = {fb, (size_t)W * H * 4, (size_t)nRays * 4, (size_t)nRays * 32, (size_t)nRays * 8, (size_t)nRays * 32};
      f.steps.push_back({"rm_post_process", [=](const Ctx &c) {
        RmPostSettings ps;
        std::memset(&ps, 0, sizeof(ps));
        ps.enableBloom = ps.enableHDR = ps.enableFXAA = 1;
        ps.exposure = 0.8f;
        return rm_post_process(dFrag, dBright, F(c, 0), W, H, &ps, S(c)); }, nullptr});
      f.steps.push_back({"rm_frames_to_rgba8", [=](const Ctx &c) { return rm_frames_to_rgba8(F(c, 0), static_cast<uint8_t *>(c.buf[1]), W, H, 1, S(c)); }, nullptr});
      f.steps.push_back({"rm_rays_order", [=](const Ctx &c) {
        return rm_rays_order(dRays[0], nRays, 4, 5, static_cast<int32_t *>(c.buf[2]), static_cast<RmRay *>(c.buf[3]), static_cast<uint64_t *>(c.buf[4]), S(c)); }, nullptr});
      f.steps.push_back({"rm_rays_restore", [=](const Ctx &c) { return rm_rays_restore(dHits, static_cast<int32_t *>(c.buf[2]), nRays, 32, c.buf[5], S(c)); }, nullptr});
      fams.push_back(f);
    }
    return run_case(fams, nullptr, nullptr);
  }

  // ================================================================================================ field
  if (g_case == "field" || g_case == "lattice") {
    // one dense and one block handle over the primitives' lattices, built here, on the main thread
    static float *dDist = nullptr, *dBDist = nullptr;
    static int32_t *dIds = nullptr, *dBIds = nullptr, *dBlocks = nullptr;
    uint32_t *dCount = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&dDist), (size_t)points * 4) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&dIds), (size_t)points * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&dBDist), (size_t)maxBlocks * 729 * 4) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&dBIds), (size_t)maxBlocks * 729 * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&dBlocks), (size_t)maxBlocks * 16) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&dCount), 256) != hipSuccess)
      return give_up("hipMalloc of the lattices failed");
    uint32_t listed = 0;
    if (rm_sdf_grid(prim.objs.data(), prim.no(), &prim.g, &prim.s, lo, step, nx, ny, nz, dDist, dIds, nullptr) != RM_OK ||
        rm_sdf_blocks_select(prim.objs.data(), prim.no(), &prim.g, &prim.s, blo, bstep, mx, my, mz, 0.0f, maxBlocks, dBlocks, dCount, nullptr) != RM_OK ||
        hipMemcpy(&listed, dCount, 4, hipMemcpyDeviceToHost) != hipSuccess || listed < 1 || listed > (uint32_t)maxBlocks ||
        rm_sdf_grid_blocks(prim.objs.data(), prim.no(), &prim.g, &prim.s, blo, bstep, mx, my, mz, dBlocks, (int)listed, dBDist, dBIds, nullptr) != RM_OK)
      return give_up(std::string("lattices: ") + rm_last_error());
    static RmField *dense = nullptr, *blocks = nullptr;
    if (rm_field_create(dDist, dIds, nx, ny, nz, lo, step, &dense) != RM_OK ||
        rm_field_create_blocks(dBDist, dBIds, dBlocks, (int)listed, mx, my, mz, blo, bstep, nullptr, &blocks) != RM_OK || hipDeviceSynchronize() != hipSuccess)
      return give_up(std::string("rm_field_create: ") + rm_last_error());
    std::vector<Family> fams;
    if (g_case == "lattice") {
      // rm_field_ambient on both handles and the handle-free lattice entries, four threads with the same family.  The block entries
      // take two lists in turn, the full one and the one without its last block, back to back on the thread's stream: the block
      // map in the stream's workspace is rebuilt behind a query that still reads the previous one.
      if (listed < 2) return give_up("the block list has " + std::to_string(listed) + " entries: the case needs two lists");
      const int nAmb = 256, full = (int)listed, shorter = (int)listed - 1;
      static std::vector<float> hemi64((size_t)3 * 64 * 4), hemi256((size_t)256 * 4);
      static float *dHemi64 = nullptr, *dHemi256 = nullptr, *dVirtual = nullptr;
      static int32_t *dVirtualIds = nullptr;
      if (rm_hemisphere_directions(64, 3, hemi64.data()) != RM_OK || rm_hemisphere_directions(256, 1, hemi256.data()) != RM_OK)
        return give_up(std::string("rm_hemisphere_directions: ") + rm_last_error());
      if (!upload(hemi64, &dHemi64) || !upload(hemi256, &dHemi256)) return finish(0, 0, 0.0, 0.0);
      // the blocks' virtual lattice as a dense one: what the Python test hands to the definition of the block entries
      const int vx = 8 * mx + 1, vy = 8 * my + 1, vz = 8 * mz + 1, vPoints = vx * vy * vz;
      if (hipMalloc(reinterpret_cast<void **>(&dVirtual), (size_t)vPoints * 4) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&dVirtualIds), (size_t)vPoints * 4) != hipSuccess)
        return give_up("hipMalloc of the virtual lattice failed");
      if (rm_sdf_grid(prim.objs.data(), prim.no(), &prim.g, &prim.s, blo, bstep, vx, vy, vz, dVirtual, dVirtualIds, nullptr) != RM_OK || hipDeviceSynchronize() != hipSuccess)
        return give_up(std::string("the virtual lattice: ") + rm_last_error());
      const int32_t head[8] = {nRays, nAmb, full, shorter, nx, ny, nz, maxBlocks};
      const float params[14] = {lo[0], lo[1], lo[2], step[0], step[1], step[2], blo[0], blo[1], blo[2], bstep[0], bstep[1], bstep[2], kAmbBias, kAmbDistance};
      if (!dump_bytes("head", head, sizeof(head)) || !dump_bytes("params", params, sizeof(params)) || !dump_vector("points", hostPoints) || !dump_vector("normals", hostNormals) || !dump_vector("rays", hostRays[0]) ||
          !dump_vector("hemi64", hemi64) || !dump_vector("hemi256", hemi256) || !dump_device("dense", dDist, (size_t)points * 4) ||
          !dump_device("dense_ids", dIds, (size_t)points * 4) || !dump_device("virtual", dVirtual, (size_t)vPoints * 4) ||
          !dump_device("virtual_ids", dVirtualIds, (size_t)vPoints * 4) || !dump_device("blocks", dBlocks, (size_t)full * 16))
        return finish(0, 0, 0.0, 0.0);
      for (int t = 0; t < 4; t++) {
        Family f;
        f.name = "lattice";
        f.rounds = 5;
        const size_t rec = (size_t)nRays * 32, amb = (size_t)nAmb * 32;
        f.bufBytes = {amb, amb, amb, amb, rec, rec, rec, rec, rec, rec, (size_t)maxBlocks * 16, 2 * sizeof(uint32_t)};
        const auto ambient = [=](RmField **h, bool soft, int b) {
          return Step{soft ? "rm_field_ambient soft" : "rm_field_ambient hard", [=](const Ctx &c) {
            return soft ? rm_field_ambient(*h, dPoints, dNormals, nAmb, dHemi64, 64, 3, kAmbBias, kAmbDistance, 0.0f, 64, RM_AMBIENT_SOFT, static_cast<RmAmbient *>(c.buf[b]), S(c))
                        : rm_field_ambient(*h, dPoints, nullptr, nAmb, dHemi256, 256, 1, kAmbBias, kAmbDistance, 0.0f, 64, RM_AMBIENT_HARD, static_cast<RmAmbient *>(c.buf[b]), S(c)); }, nullptr}; };
        const auto sampleBlocks = [=](int count, int b) {
          return Step{"rm_sdf_sample_blocks", [=](const Ctx &c) {
            return rm_sdf_sample_blocks(dPoints, nRays, dBDist, dBIds, dBlocks, count, mx, my, mz, blo, bstep, static_cast<RmFieldSample *>(c.buf[b]), S(c)); }, nullptr}; };
        const auto traceBlocks = [=](int count, int b) {
          return Step{"rm_sdf_trace_blocks", [=](const Ctx &c) {
            return rm_sdf_trace_blocks(dRays[0], nRays, dBDist, dBIds, dBlocks, count, mx, my, mz, blo, bstep, 0.0f, 128, 0u, static_cast<RmRayHit *>(c.buf[b]), S(c)); }, nullptr}; };
        f.steps = {ambient(&dense, true, 0), ambient(&blocks, true, 1), ambient(&dense, false, 2), ambient(&blocks, false, 3),
                   Step{"rm_sdf_sample", [=](const Ctx &c) { return rm_sdf_sample(dPoints, nRays, dDist, dIds, nx, ny, nz, lo, step, static_cast<RmFieldSample *>(c.buf[4]), S(c)); }, nullptr},
                   Step{"rm_sdf_trace", [=](const Ctx &c) { return rm_sdf_trace(dRays[0], nRays, dDist, dIds, nx, ny, nz, lo, step, 0.0f, 128, 0u, static_cast<RmRayHit *>(c.buf[5]), S(c)); }, nullptr},
                   sampleBlocks(full, 6), sampleBlocks(shorter, 7), traceBlocks(full, 8), traceBlocks(shorter, 9),
                   Step{"rm_sdf_blocks_select_pruned", [=](const Ctx &c) {
                     return rm_sdf_blocks_select_pruned(prim.objs.data(), prim.no(), &prim.g, &prim.s, blo, bstep, mx, my, mz, 0.0f, 1.0f, 1.0f, maxBlocks, static_cast<int32_t *>(c.buf[10]),
                                                        static_cast<uint32_t *>(c.buf[11]), S(c)); }, nullptr}};
        if (t == 0) f.dump = dump_buffers("lattice");
        fams.push_back(f);
      }
    }
    for (int t = 0; t < 4 && g_case == "field"; t++) {
      Family f;
      f.name = "queries";
      f.rounds = 5;
      f.bufBytes.assign(10, (size_t)nRays * 32);
      const auto sample = [nRays](RmField **h, int b) { return Step{"rm_field_sample", [=](const Ctx &c) { return rm_field_sample(*h, dPoints, nRays, static_cast<RmFieldSample *>(c.buf[b]), S(c)); }, nullptr}; };
      const auto trace = [nRays](RmField **h, unsigned mode, int b) {
        return Step{"rm_field_trace", [=](const Ctx &c) { return rm_field_trace(*h, dRays[0], nRays, 0.0f, 128, mode, static_cast<RmRayHit *>(c.buf[b]), S(c)); }, nullptr}; };
      f.steps = {sample(&dense, 0), trace(&dense, RM_TRACE_CLOSEST, 1), sample(&blocks, 2), trace(&blocks, RM_TRACE_CLOSEST, 3), trace(&dense, RM_TRACE_NO_NORMAL, 4),
                 trace(&blocks, RM_TRACE_NO_NORMAL, 5), trace(&dense, RM_TRACE_OCCLUSION, 6), trace(&blocks, RM_TRACE_OCCLUSION, 7), sample(&dense, 8), sample(&blocks, 9)};
      fams.push_back(f);
    }
    const int rc = run_case(fams, nullptr, nullptr);
    rm_field_destroy(dense);
    rm_field_destroy(blocks);
    return rc;
  }

  // ================================================================================================ light
  if (g_case == "light") {
    const int nProbes = kGridDims[0] * kGridDims[1] * kGridDims[2];
    // read-only inputs, built here on the main thread: the grid's positions, the two direction tables, the depth weights
    static std::vector<float> gridPos((size_t)nProbes * 4);
    for (int k = 0; k < kGridDims[2]; k++)
      for (int j = 0; j < kGridDims[1]; j++)
        for (int i = 0; i < kGridDims[0]; i++) {
          float *p = &gridPos[(size_t)(i + kGridDims[0] * (j + kGridDims[1] * k)) * 4];
          p[0] = kGridOrigin[0] + (float)i * kGridStep[0]; p[1] = kGridOrigin[1] + (float)j * kGridStep[1]; p[2] = kGridOrigin[2] + (float)k * kGridStep[2];
          p[3] = 1.0f;
        }
    static std::vector<RmProbeDir> dirs64(3 * 64), dirs128(128);
    static std::vector<float> weights64((size_t)3 * 64 * RM_PROBE_DEPTH_TEXELS);
    if (rm_sphere_directions(64, 3, dirs64.data()) != RM_OK || rm_sphere_directions(128, 1, dirs128.data()) != RM_OK ||
        rm_probe_depth_weights(dirs64.data(), 64, 3, 50.0f, weights64.data()) != RM_OK)
      return give_up(std::string("direction tables: ") + rm_last_error());
    static float *dPos = nullptr, *dWeights = nullptr;
    static RmProbeDir *dDirs64 = nullptr, *dDirs128 = nullptr;
    if (!upload(gridPos, &dPos) || !upload(dirs64, &dDirs64) || !upload(dirs128, &dDirs128) || !upload(weights64, &dWeights)) return finish(0, 0, 0.0, 0.0);
    // per scene the shared grid, baked at K = 64, and its depth records
    static RmLightProbe *dGrid[2] = {nullptr, nullptr};
    static RmProbeDepth *dDepth[2] = {nullptr, nullptr};
    for (int v = 0; v < 2; v++) {
      const SceneData &s = *two[v];
      if (hipMalloc(reinterpret_cast<void **>(&dGrid[v]), (size_t)nProbes * sizeof(RmLightProbe)) != hipSuccess ||
          hipMalloc(reinterpret_cast<void **>(&dDepth[v]), (size_t)nProbes * sizeof(RmProbeDepth)) != hipSuccess)
        return give_up("hipMalloc of the shared grid failed");
      if (rm_light_probes(dPos, nProbes, dDirs64, 64, 3, kLightFar, s.objs.data(), s.no(), s.lights.data(), s.nl(), &s.g, &s.s, nullptr, dGrid[v], nullptr) != RM_OK ||
          rm_light_probes_depth(dPos, nProbes, dDirs64, dWeights, 64, 3, kDepthDistance, s.objs.data(), s.no(), &s.g, &s.s, dDepth[v], nullptr) != RM_OK ||
          hipDeviceSynchronize() != hipSuccess)
        return give_up(std::string("the shared grid: ") + rm_last_error());
    }
    // the layer families' table (terrain + sea under the sky, two times of day), its rays and the noise texture
    static SceneData land[2];
    static std::vector<uint8_t> noise;
    static std::vector<RmRay> landRays((size_t)nRays);
    static RmRay *dLandRays = nullptr;
    static RmResources res;
    noise_texture(&noise);
    uint8_t *dNoise = nullptr;
    if (!layers_scene(64, 64, 0.7f, &land[0]) || !layers_scene(64, 64, 1.9f, &land[1]) || !upload(noise, &dNoise)) return finish(0, 0, 0.0, 0.0);
    if (rm_camera_rays(&land[0].cam, 64, 64, nullptr, nRays, landRays.data()) != RM_OK) return give_up(std::string("rm_camera_rays: ") + rm_last_error());
    if (!upload(landRays, &dLandRays)) return finish(0, 0, 0.0, 0.0);
    std::memset(&res, 0, sizeof(res));
    res.noise.pixels = dNoise; res.noise.width = 256; res.noise.height = 256;
    // the inputs, for the Python test that holds the serial records to each entry's definition
    const int32_t head[4] = {nRays, nProbes, kGridDims[0] | kGridDims[1] << 8 | kGridDims[2] << 16, 0};
    const float params[10] = {kGridOrigin[0], kGridOrigin[1], kGridOrigin[2], kGridStep[0], kGridStep[1], kGridStep[2], kLightFar, kDepthDistance, kNormalBias, kStrength};
    bool dumped = dump_bytes("head", head, sizeof(head)) && dump_bytes("params", params, sizeof(params)) && dump_vector("positions", gridPos) &&
                  dump_vector("dirs64", dirs64) && dump_vector("dirs128", dirs128) && dump_vector("weights64", weights64) && dump_vector("points", hostPoints) &&
                  dump_vector("normals", hostNormals);
    for (int v = 0; v < 2 && dumped; v++)
      dumped = dump_vector("rays_v" + std::to_string(v), hostRays[v]) && dump_device("grid_v" + std::to_string(v), dGrid[v], (size_t)nProbes * sizeof(RmLightProbe)) &&
               dump_device("depth_v" + std::to_string(v), dDepth[v], (size_t)nProbes * sizeof(RmProbeDepth)) &&
               dump_frame("scene_v" + std::to_string(v), *two[v], Bytes(), nullptr, ".tables");
    if (!dumped) return finish(0, 0, 0.0, 0.0);

    const size_t probeBytes = (size_t)nProbes * sizeof(RmLightProbe), depthBytes = (size_t)nProbes * sizeof(RmProbeDepth), lightBytes = (size_t)nRays * sizeof(RmGridLight);
    const auto done = [](HostArgs &a, int rc) { a.spoil(); return rc; };  // the call has returned: its host arguments are overwritten
    const auto probes = [=](RmProbeDir **dirs, int K, int sets, int b) {
      return Step{"rm_light_probes", [=](const Ctx &c) {
        HostArgs &a = host_args(*two[c.variant & 1], nullptr, nullptr, 0);
        return done(a, rm_light_probes(dPos, nProbes, *dirs, K, sets, kLightFar, a.objs.data(), a.no(), a.lights.data(), a.nl(), &a.g, &a.s, nullptr, static_cast<RmLightProbe *>(c.buf[b]), S(c))); }, nullptr}; };
    std::vector<Family> fams;
    {
      Family f; f.name = "probes_64"; f.rounds = 8; f.variants = 2; f.bufBytes = {probeBytes};
      f.steps = {probes(&dDirs64, 64, 3, 0)};
      f.dump = dump_buffers(f.name);
      fams.push_back(f);
    }
    {
      Family f; f.name = "probes_128"; f.rounds = 8; f.variants = 2; f.bufBytes = {probeBytes};
      f.steps = {probes(&dDirs128, 128, 1, 0)};
      f.dump = dump_buffers(f.name);
      fams.push_back(f);
    }
    {
      // the lookup reads the round's own depth records, behind their bake on the same stream with no synchronise between the two
      Family f; f.name = "depth"; f.rounds = 8; f.variants = 2; f.bufBytes = {depthBytes, lightBytes};
      f.steps.push_back({"rm_light_probes_depth", [=](const Ctx &c) {
        HostArgs &a = host_args(*two[c.variant], nullptr, nullptr, 0);
        return done(a, rm_light_probes_depth(dPos, nProbes, dDirs64, dWeights, 64, 3, kDepthDistance, a.objs.data(), a.no(), &a.g, &a.s, static_cast<RmProbeDepth *>(c.buf[0]), S(c))); }, nullptr});
      f.steps.push_back({"rm_light_grid_irradiance_visible", [=](const Ctx &c) {
        HostArgs &a = host_args(*two[c.variant], nullptr, nullptr, 0);
        return done(a, rm_light_grid_irradiance_visible(dGrid[c.variant], static_cast<RmProbeDepth *>(c.buf[0]), a.dims, a.origin, a.step, dPoints, dNormals, nRays, RM_LIGHT_GRID_FACING, kNormalBias,
                                                        static_cast<RmGridLight *>(c.buf[1]), S(c))); }, nullptr});
      f.dump = dump_buffers(f.name);
      fams.push_back(f);
    }
    {
      Family f; f.name = "lookups"; f.rounds = 8; f.variants = 2; f.bufBytes = {lightBytes, lightBytes, lightBytes};
      const auto plain = [=](uint32_t flags, int b) {
        return Step{"rm_light_grid_irradiance", [=](const Ctx &c) {
          HostArgs &a = host_args(*two[c.variant], nullptr, nullptr, 0);
          return done(a, rm_light_grid_irradiance(dGrid[c.variant], a.dims, a.origin, a.step, dPoints, dNormals, nRays, flags, static_cast<RmGridLight *>(c.buf[b]), S(c))); }, nullptr}; };
      f.steps = {plain(RM_LIGHT_GRID_FACING, 0), plain(0u, 1)};
      f.steps.push_back({"rm_light_grid_irradiance_visible", [=](const Ctx &c) {
        HostArgs &a = host_args(*two[c.variant], nullptr, nullptr, 0);
        return done(a, rm_light_grid_irradiance_visible(dGrid[c.variant], dDepth[c.variant], a.dims, a.origin, a.step, dPoints, dNormals, nRays, RM_LIGHT_GRID_FACING, kNormalBias,
                                                        static_cast<RmGridLight *>(c.buf[2]), S(c))); }, nullptr});
      f.dump = dump_buffers(f.name);
      fams.push_back(f);
    }
    {
      // variant: bit 0 the scene, bit 1 whether the grid comes with its depth records — one round in two of each scene
      Family f; f.name = "indirect"; f.rounds = 8; f.variants = 4; f.bufBytes = {(size_t)nRays * 16, probeBytes};
      f.steps.push_back({"rm_shade_rays_indirect", [=](const Ctx &c) {
        const int v = c.variant & 1;
        HostArgs &a = host_args(*two[v], dGrid[v], (c.variant & 2) ? dDepth[v] : nullptr, RM_LIGHT_GRID_FACING);
        return done(a, rm_shade_rays_indirect(dRays[v], nRays, kLightFar, a.objs.data(), a.no(), a.lights.data(), a.nl(), &a.g, &a.s, nullptr, &a.grid, F(c, 0), S(c))); }, nullptr});
      f.steps.push_back({"rm_light_probes_indirect", [=](const Ctx &c) {
        const int v = c.variant & 1;
        HostArgs &a = host_args(*two[v], dGrid[v], (c.variant & 2) ? dDepth[v] : nullptr, RM_LIGHT_GRID_FACING);
        return done(a, rm_light_probes_indirect(dPos, nProbes, dDirs64, 64, 3, kLightFar, a.objs.data(), a.no(), a.lights.data(), a.nl(), &a.g, &a.s, nullptr, &a.grid,
                                                static_cast<RmLightProbe *>(c.buf[1]), S(c))); }, nullptr});
      f.dump = dump_buffers(f.name);
      fams.push_back(f);
    }
    {
      // three staged blocks on one stream with two device-side dependencies and no synchronise: a bake, a second bounce that reads
      // it through an RmLightGridRef, rays lit by the second bounce
      Family f; f.name = "bounce_chain"; f.rounds = 8; f.variants = 2; f.bufBytes = {probeBytes, probeBytes, (size_t)nRays * 16};
      f.steps = {probes(&dDirs64, 64, 3, 0)};
      f.steps.push_back({"rm_light_probes_indirect", [=](const Ctx &c) {
        HostArgs &a = host_args(*two[c.variant], static_cast<RmLightProbe *>(c.buf[0]), nullptr, RM_LIGHT_GRID_FACING);
        return done(a, rm_light_probes_indirect(dPos, nProbes, dDirs64, 64, 3, kLightFar, a.objs.data(), a.no(), a.lights.data(), a.nl(), &a.g, &a.s, nullptr, &a.grid,
                                                static_cast<RmLightProbe *>(c.buf[1]), S(c))); }, nullptr});
      f.steps.push_back({"rm_shade_rays_indirect", [=](const Ctx &c) {
        HostArgs &a = host_args(*two[c.variant], static_cast<RmLightProbe *>(c.buf[1]), nullptr, RM_LIGHT_GRID_FACING);
        return done(a, rm_shade_rays_indirect(dRays[c.variant], nRays, kLightFar, a.objs.data(), a.no(), a.lights.data(), a.nl(), &a.g, &a.s, nullptr, &a.grid, F(c, 2), S(c))); }, nullptr});
      f.dump = dump_buffers(f.name);
      fams.push_back(f);
    }
    {
      Family f; f.name = "layers"; f.rounds = 8; f.variants = 2; f.bufBytes = {(size_t)nRays * 16, (size_t)nRays * 16, (size_t)nRays * 32};
      f.steps.push_back({"rm_shade_rays_layers", [=](const Ctx &c) { const SceneData &s = land[c.variant];
        return rm_shade_rays_layers(dLandRays, nRays, kLightFar, 64, s.objs.data(), s.no(), s.lights.data(), s.nl(), &s.g, &s.s, &res, F(c, 0), F(c, 1), S(c)); }, nullptr});
      f.steps.push_back({"rm_trace_rays_layers", [=](const Ctx &c) { const SceneData &s = land[c.variant];
        return rm_trace_rays_layers(dLandRays, nRays, 64, s.objs.data(), s.no(), &s.g, &s.s, RM_TRACE_CLOSEST, static_cast<RmRayHit *>(c.buf[2]), S(c)); }, nullptr});
      fams.push_back(f);
    }
    {
      // the single-frame ring and the tuner beside the batch ring: the frame as rm_render_res and rm_render_ex give it, then as the
      // two shards of a row-tile partition, de-interleaved, converted to 8 bits both ways round, and one post pass of a batch.
      // Buffers: 0 frame, 1 frame and 2 bright of rm_render_ex, 3 the two shards' slots, 4 the de-interleaved frame, 5 the slots
      // in 8 bits, 6 their de-interleaved frame, 7 buffer 4 in 8 bits, 8 the post pass.  The serial frame is dumped for the oracle.
      const int tileRows = 8, slotRows = rm_gather_slot_rows(bulb.H, tileRows, 2);
      if (slotRows < rm_shard_rows(bulb.H, tileRows, 0, 2) || slotRows < rm_shard_rows(bulb.H, tileRows, 1, 2) || slotRows > bulb.H)
        return give_up("rm_gather_slot_rows: " + std::to_string(slotRows) + " rows");
      const size_t slotFloats = (size_t)slotRows * bulb.W * 4, px = (size_t)bulb.W * bulb.H;
      Family f = render_family("render", &bulb, 4, nullptr, 0, false, 1, nullptr);
      f.bufBytes = {px * 16, px * 16, px * 16, 2 * slotFloats * 4, px * 16, 2 * slotFloats, px * 4, px * 4, px * 16};
      f.steps.push_back({"rm_render_ex", [](const Ctx &c) {
        return rm_render_ex(&bulb.cam, bulb.objs.data(), bulb.no(), bulb.lights.data(), bulb.nl(), &bulb.g, &bulb.s, nullptr, 0, bulb.W, bulb.H, 0, bulb.H, F(c, 1), F(c, 2), S(c)); }, nullptr});
      f.steps.push_back({"rm_render_tiles", [=](const Ctx &c) {
        return rm_render_tiles(&bulb.cam, bulb.objs.data(), bulb.no(), bulb.lights.data(), bulb.nl(), &bulb.g, &bulb.s, bulb.W, bulb.H, tileRows, 0, 2, F(c, 3), nullptr, S(c)); }, nullptr});
      f.steps.push_back({"rm_render_tiles_res", [=](const Ctx &c) {
        return rm_render_tiles_res(&bulb.cam, bulb.objs.data(), bulb.no(), bulb.lights.data(), bulb.nl(), &bulb.g, &bulb.s, nullptr, bulb.W, bulb.H, tileRows, 1, 2, F(c, 3) + slotFloats,
                                   nullptr, S(c)); }, nullptr});
      f.steps.push_back({"rm_deinterleave", [=](const Ctx &c) { return rm_deinterleave(F(c, 3), F(c, 4), bulb.W, bulb.H, tileRows, 2, slotRows, S(c)); }, nullptr});
      f.steps.push_back({"rm_tiles_to_rgba8", [=](const Ctx &c) { return rm_tiles_to_rgba8(F(c, 3), static_cast<uint8_t *>(c.buf[5]), bulb.W, 2 * slotRows, S(c)); }, nullptr});
      f.steps.push_back({"rm_deinterleave_rgba8", [=](const Ctx &c) {
        return rm_deinterleave_rgba8(static_cast<uint8_t *>(c.buf[5]), static_cast<uint8_t *>(c.buf[6]), bulb.W, bulb.H, tileRows, 2, slotRows, 1, S(c)); }, nullptr});
      f.steps.push_back({"rm_frame_to_rgba8", [](const Ctx &c) { return rm_frame_to_rgba8(F(c, 4), static_cast<uint8_t *>(c.buf[7]), bulb.W, bulb.H, S(c)); }, nullptr});
      f.steps.push_back({"rm_post_process_batch", [](const Ctx &c) {
        RmPostSettings ps;
        std::memset(&ps, 0, sizeof(ps));
        ps.enableBloom = ps.enableHDR = ps.enableFXAA = 1;
        ps.exposure = 0.8f;
        return rm_post_process_batch(F(c, 1), F(c, 2), F(c, 8), bulb.W, bulb.H, 1, &ps, 1, S(c)); }, nullptr});
      f.dump = [](int v, const std::vector<Bytes> &e) { return dump_frame("render", bulb, e[0], nullptr, ".tables") && dump_buffers("render")(v, e); };
      fams.push_back(f);
    }
    return run_case(fams, nullptr, nullptr);
  }

  // ================================================================================================ release
  if (g_case == "release") {
    static SceneData big, menger;
    if (!primitives_scene(256, 128, &big) || !menger_scene(scenes, 96, 61, &menger)) return finish(0, 0, 0.0, 0.0);
    const size_t bigBytes = frame_bytes(big);
    static float *dFrag = nullptr, *dBright = nullptr, *dSphere = nullptr;
    const int sx = 33, sy = 35, sz = 70, sPoints = sx * sy * sz, sCells = (sx - 1) * (sy - 1) * (sz - 1);
    static const float slo[3] = {-0.8f, -0.8f, -0.8f}, sstep[3] = {1.6f / 32.0f, 1.6f / 34.0f, 1.6f / 69.0f};
    static std::vector<RmObject> sphere = {primitive(RM_SPHERE, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 1.0f)};
    if (hipMalloc(reinterpret_cast<void **>(&dFrag), bigBytes) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&dBright), bigBytes) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&dSphere), (size_t)sPoints * 4) != hipSuccess)
      return give_up("hipMalloc of the inputs failed");
    if (rm_render(&big.cam, big.objs.data(), big.no(), big.lights.data(), big.nl(), &big.g, &big.s, big.W, big.H, 0, big.H, dFrag, dBright, nullptr) != RM_OK ||
        rm_sdf_grid(sphere.data(), 1, &prim.g, &prim.s, slo, sstep, sx, sy, sz, dSphere, nullptr, nullptr) != RM_OK || hipDeviceSynchronize() != hipSuccess)
      return give_up(std::string("inputs: ") + rm_last_error());
    if (rm_set_kernel_path(5) != RM_OK) return give_up(std::string("rm_set_kernel_path: ") + rm_last_error());
    std::vector<Family> fams;
    {
      Family f; f.name = "post"; f.rounds = 40; f.bufBytes = {bigBytes};
      f.steps.push_back({"rm_post_process", [](const Ctx &c) {
        RmPostSettings ps;
        std::memset(&ps, 0, sizeof(ps));
        ps.enableBloom = ps.enableHDR = ps.enableFXAA = 1;
        ps.exposure = 0.8f;
        return rm_post_process(dFrag, dBright, F(c, 0), big.W, big.H, &ps, S(c)); }, nullptr});
      fams.push_back(f);
    }
    {
      const size_t fb = (size_t)W * H * 16;
      Family f; f.name = "adaptive"; f.rounds = 40; f.bufBytes = {fb, fb, (size_t)W * H, sizeof(uint32_t)};
      f.steps.push_back({"rm_render_adaptive", [](const Ctx &c) {
        return rm_render_adaptive(&prim.cam, &prim.g, 1, 1, prim.objs.data(), prim.no(), prim.lights.data(), prim.nl(), &prim.s, nullptr, prim.W, prim.H, 2, 0.05f, F(c, 0), F(c, 1),
                                  static_cast<uint8_t *>(c.buf[2]), static_cast<uint32_t *>(c.buf[3]), S(c)); }, nullptr});
      fams.push_back(f);
    }
    {
      // the surface of a sphere of radius 0.5 crosses a few thousand of the 75 072 cells: capacities of a fifth of them are ample,
      // and a count above a capacity would only leave the tail unstored, in the serial pass and on the thread alike
      const int maxV = sCells / 5, maxQ = sCells / 5;
      Family f; f.name = "mesh_wavefront"; f.rounds = 20;
      f.bufBytes = {(size_t)maxV * 16, (size_t)maxQ * 16, 2 * sizeof(uint32_t), frame_bytes(menger)};
      f.steps.push_back({"rm_sdf_mesh", [=](const Ctx &c) {
        return rm_sdf_mesh(dSphere, nullptr, sx, sy, sz, slo, sstep, 0.0f, maxV, maxQ, F(c, 0), nullptr, static_cast<int32_t *>(c.buf[1]), static_cast<uint32_t *>(c.buf[2]), S(c)); },
        [=](const Ctx &c) {
          uint32_t n[2] = {0, 0};
          HIP_TRY(hipMemcpy(n, c.buf[2], 8, hipMemcpyDeviceToHost));
          if (n[0] < 50 || n[0] > (uint32_t)maxV || n[1] > (uint32_t)maxQ) { mismatch("sphere mesh: " + std::to_string(n[0]) + " vertices, " + std::to_string(n[1]) + " quads"); return false; }
          return true;
        }});
      f.steps.push_back({"rm_render", [](const Ctx &c) {
        return rm_render(&menger.cam, menger.objs.data(), menger.no(), menger.lights.data(), menger.nl(), &menger.g, &menger.s, menger.W, menger.H, 0, menger.H, F(c, 3), nullptr, S(c)); },
        [](const Ctx &) {
          if (rm_debug_last_path() != 5) { mismatch("the sponge's serial frame ran path " + std::to_string(rm_debug_last_path()) + ", not the wavefront pipeline"); return false; }
          return true;
        }});
      f.dump = [](int, const std::vector<Bytes> &e) { return dump_frame("wavefront", menger, e[3], nullptr); };
      fams.push_back(f);
    }
    {
      Family f; f.name = "release"; f.rounds = 10;
      f.steps.push_back({"rm_release_workspaces", [](const Ctx &c) {
        unsigned long long freed = 0;
        const int rc = rm_release_workspaces(&freed);
        if (!c.serial) std::this_thread::sleep_for(std::chrono::milliseconds(2));
        return rc; }, nullptr});
      fams.push_back(f);
    }
    const auto last = [] {
      unsigned long long freed = 0;
      if (rm_release_workspaces(&freed) != RM_OK) { mismatch(std::string("the final rm_release_workspaces: ") + rm_last_error()); return false; }
      return true;
    };
    return run_case(fams, nullptr, last);
  }

  return give_up("unknown case " + g_case);
}
