// The host-only half of the library called from eight real threads at once (TEST INFRASTRUCTURE), built with
// g++ -fsanitize=thread: the scenefile loader and the camera builders, the image readers, the rm_debug_* functions that keep a
// static SceneBlock behind a static mutex (rm_frame.cpp), and the thread-local text of rm_last_error (rm_host.cpp).  Every
// result a thread gets is memcmp'd against the result of the same call made alone, before the threads start; ThreadSanitizer
// reports the data race of a lock or a thread_local that went missing.  No GPU, no HIP.
// Usage: host_threads <scenes dir>      — prints "host_threads ok" as its last line, exit status 0.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/raymarcher_amd.h"
#include "../../raymarcher_amd/csrc/rm_internal.h"

// the two helpers the launcher (rm_launcher.hip) defines for the host files
namespace rm {
bool device_accessible(const void *) { return false; }
int require_device_pointers(std::initializer_list<std::pair<const char *, const void *>>) { return RM_ERR_INVALID_ARGUMENT; }
}  // namespace rm

static const int kThreads = 8;
static const int kDebugCalls = 2000;  // per function and thread
static const int kErrorCalls = 2000;

static void walk(const std::string &dir, std::vector<std::string> &out) {
  DIR *d = opendir(dir.c_str());
  if (!d) return;
  while (dirent *e = readdir(d)) {
    std::string n = e->d_name;
    if (n == "." || n == "..") continue;
    std::string p = dir + "/" + n;
    struct stat st;
    if (stat(p.c_str(), &st) != 0) continue;
    if (S_ISDIR(st.st_mode)) walk(p, out); else out.push_back(p);
  }
  closedir(d);
}
static bool ends(const std::string &s, const char *suf) { size_t n = strlen(suf); return s.size() >= n && s.compare(s.size() - n, n, suf) == 0; }

class Barrier {
 public:
  explicit Barrier(int n) : n_(n) {}
  void wait() {
    std::unique_lock<std::mutex> lk(mu_);
    const int gen = gen_;
    if (++count_ == n_) { count_ = 0; gen_++; cv_.notify_all(); return; }
    cv_.wait(lk, [&] { return gen != gen_; });
  }
 private:
  std::mutex mu_;
  std::condition_variable cv_;
  int n_, count_ = 0, gen_ = 0;
};

typedef std::vector<uint8_t> Bytes;
static void put(Bytes &b, const void *p, size_t n) { const uint8_t *q = static_cast<const uint8_t *>(p); b.insert(b.end(), q, q + n); }
static void put_int(Bytes &b, int v) { put(b, &v, sizeof(v)); }

// failures of all threads; the first few are printed
static std::mutex g_failMu;
static int g_failures = 0;
static void fail(int tid, const std::string &what) {
  std::lock_guard<std::mutex> lk(g_failMu);
  if (g_failures++ < 10) fprintf(stderr, "thread %d: %s\n", tid, what.c_str());
}

// wall-clock stamps of the phases, taken by thread 0 behind each barrier (and by main after the join)
static std::chrono::steady_clock::time_point g_stamp[5];
static void stamp(int tid, int k) { if (tid == 0) g_stamp[k] = std::chrono::steady_clock::now(); }

// ---- 1. the loader: everything a host reads off a scenefile, as one byte record
static Bytes scene_record(const std::string &path, int *loaded) {
  Bytes b;
  RmScene *sc = nullptr;
  const int st = rm_scene_load(path.c_str(), &sc);
  put_int(b, st);
  if (st != RM_OK || !sc) {
    const char *e = rm_last_error();  // the refusal's text is this thread's own
    put(b, e, strlen(e));
    return b;
  }
  if (loaded) ++*loaded;
  const int no = rm_scene_num_objects(sc), nl = rm_scene_num_lights(sc);
  put_int(b, no);
  put_int(b, nl);
  put(b, rm_scene_objects(sc), sizeof(RmObject) * (size_t)no);
  put(b, rm_scene_lights(sc), sizeof(RmLight) * (size_t)nl);
  for (int i = 0; i < no; i++) { const char *t = rm_scene_object_texture(sc, i); if (t) put(b, t, strlen(t)); put_int(b, i); }
  RmHostSettings hs;
  rm_host_settings_default(&hs);
  RmGlobals g;
  std::memset(&g, 0, sizeof(g));
  put_int(b, rm_scene_globals(sc, &hs, &g));
  put(b, &g, sizeof(g));
  RmCameraData cd;
  std::memset(&cd, 0, sizeof(cd));
  const int cs = rm_scene_camera_data(sc, &cd);
  put_int(b, cs);
  put(b, &cd, sizeof(cd));
  if (cs == RM_OK) {
    float view[16] = {0}, proj[16] = {0};
    RmCamera cam, lens[5];
    std::memset(&cam, 0, sizeof(cam));
    std::memset(lens, 0, sizeof(lens));
    put_int(b, rm_camera_build(&cd, 640, 360, 0.1f, 100.0f, view, proj, &cam));
    put(b, view, sizeof(view));
    put(b, proj, sizeof(proj));
    put(b, &cam, sizeof(cam));
    put_int(b, rm_camera_lens_samples(&cd, 640, 360, 0.1f, 100.0f, 0.05f, 3.0f, 5, lens));
    put(b, lens, sizeof(lens));
  }
  rm_scene_free(sc);
  return b;
}

// ---- 2. the rm_debug_* functions with static scratch: one input set per (thread, variation)
struct DebugInput {
  RmCamera cam;
  std::vector<RmObject> objs;
  std::vector<RmLight> lights;
  RmGlobals g;
};
struct DebugOutput {
  int stPlanes, stCull, stPrep, plain;
  float planes[48], cull[14], prep[8 * RM_MAX_LIGHTS];
};
static void debug_calls(const DebugInput &in, DebugOutput *out, int which) {
  const int no = (int)in.objs.size(), nl = (int)in.lights.size();
  if (which < 0 || which == 0) out->stPlanes = rm_debug_ray_planes(&in.cam, out->planes);
  if (which < 0 || which == 1) out->stCull = rm_debug_cull_bounds(in.objs.data(), no, &in.g, out->cull);
  if (which < 0 || which == 2) out->stPrep = rm_debug_light_prep(in.objs.data(), no, in.lights.data(), nl, out->prep);
  if (which < 0 || which == 3) out->plain = rm_debug_bulb_plain(in.objs.data(), no, &in.g);
}

// ---- 3. the image readers
static Bytes image_record(const std::string &path, int flip) {
  Bytes b;
  {
    uint8_t *px = nullptr;
    int w = 0, h = 0;
    const int st = rm_image_load(path.c_str(), flip, &px, &w, &h);
    put_int(b, st);
    if (st != RM_OK || !px) return b;
    put_int(b, w);
    put_int(b, h);
    uint64_t hash = 1469598103934665603ull;  // FNV-1a over every byte
    for (size_t i = 0; i < (size_t)w * (size_t)h * 4; i++) hash = (hash ^ px[i]) * 1099511628211ull;
    put(b, &hash, sizeof(hash));
    rm_image_free(px);
  }
  return b;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: host_threads <scenes dir>\n"); return 2; }
  std::vector<std::string> files, scenes, images;
  walk(argv[1], files);
  std::sort(files.begin(), files.end());
  for (auto &f : files) {
    if (ends(f, ".json")) scenes.push_back(f);
    else if (ends(f, ".png") || ends(f, ".jpg") || ends(f, ".jpeg") || ends(f, ".gif")) {
      struct stat st;
      // PNG, JPEG and GIF are all among the files below 100 KB; a 2.6-megapixel PNG per thread would spend the run in zlib
      if (stat(f.c_str(), &st) == 0 && st.st_size <= 100000) images.push_back(f);
    }
  }
  if (scenes.empty() || images.empty()) { fprintf(stderr, "no inputs under %s\n", argv[1]); return 2; }

  // ---------------------------------------------------------------- the serial pass: every call made alone
  int loaded = 0;
  std::vector<Bytes> sceneRef, imageRef;
  for (auto &s : scenes) sceneRef.push_back(scene_record(s, &loaded));
  for (size_t i = 0; i < images.size(); i++) imageRef.push_back(image_record(images[i], (int)(i & 1)));  // bottom-up and top-down rows in turn

  // debug inputs: the tables of the scenefiles that load, moved by a per-thread offset; cameras of per-thread frame sizes
  const int kVar = 12;
  std::vector<std::vector<DebugInput>> dbgIn(kThreads);
  std::vector<std::vector<DebugOutput>> dbgRef(kThreads);
  {
    std::vector<RmScene *> open;
    for (auto &s : scenes) { RmScene *sc = nullptr; if (rm_scene_load(s.c_str(), &sc) == RM_OK && sc) open.push_back(sc); }
    if (open.empty()) { fprintf(stderr, "no scenefile loads\n"); return 2; }
    for (int t = 0; t < kThreads; t++) {
      for (int v = 0; v < kVar; v++) {
        RmScene *sc = open[(size_t)(t * kVar + v * 5) % open.size()];
        DebugInput in;
        RmCameraData cd;
        std::memset(&in.cam, 0, sizeof(in.cam));
        if (rm_scene_camera_data(sc, &cd) != RM_OK || rm_camera_build(&cd, 320 + 16 * t, 200 + 8 * v, 0.1f, 100.0f, nullptr, nullptr, &in.cam) != RM_OK) {
          in.cam.invProjView[0] = in.cam.invProjView[5] = in.cam.invProjView[10] = in.cam.invProjView[15] = 1.0f + (float)t;
          in.cam.initialFar = 100.0f;
        }
        RmHostSettings hs;
        rm_host_settings_default(&hs);
        if (v % 3 == 1) { hs.juliaSeed[0] = 0.1f * (float)(t + 1); hs.power = 6.0f; }
        rm_scene_globals(sc, &hs, &in.g);
        const int no = rm_scene_num_objects(sc), nl = std::min(rm_scene_num_lights(sc), RM_MAX_LIGHTS);
        const float move[3] = {0.25f * (float)t, -0.125f * (float)v, 0.0625f * (float)(t + v)};
        for (int i = 0; i < no && i < RM_MAX_OBJECTS; i++) {
          RmObject o;
          if (rm_object_translated(rm_scene_objects(sc) + i, move, &o) != RM_OK) o = rm_scene_objects(sc)[i];
          in.objs.push_back(o);
        }
        in.lights.assign(rm_scene_lights(sc), rm_scene_lights(sc) + nl);
        DebugOutput out;
        std::memset(&out, 0, sizeof(out));
        debug_calls(in, &out, -1);
        dbgIn[t].push_back(in);
        dbgRef[t].push_back(out);
      }
    }
    for (RmScene *sc : open) rm_scene_free(sc);
  }

  // ---------------------------------------------------------------- eight threads
  Barrier barrier(kThreads);
  std::vector<std::thread> threads;
  for (int tid = 0; tid < kThreads; tid++) {
    threads.emplace_back([&, tid] {
      // 1. the loader, every thread in an order of its own
      std::vector<size_t> order(scenes.size());
      for (size_t i = 0; i < order.size(); i++) order[i] = (i * 7 + (size_t)tid * 11) % order.size();  // 7 and 52 are coprime
      if (tid & 1) std::reverse(order.begin(), order.end());
      barrier.wait();
      stamp(tid, 0);
      for (size_t i : order)
        if (scene_record(scenes[i], nullptr) != sceneRef[i]) fail(tid, "scenefile record differs from the serial one: " + scenes[i]);

      // 2. the functions with static scratch behind a mutex, one function at a time so that all eight threads meet in it
      for (int which = 0; which < 4; which++) {
        barrier.wait();
        if (which == 0) stamp(tid, 1);
        for (int c = 0; c < kDebugCalls; c++) {
          const int v = c % kVar;
          DebugOutput out = dbgRef[tid][v];  // the fields the call does not write keep the reference's bytes
          if (which == 0) std::memset(out.planes, 0xA5, sizeof(out.planes));
          if (which == 1) std::memset(out.cull, 0xA5, sizeof(out.cull));
          if (which == 2) std::memset(out.prep, 0xA5, sizeof(float) * 8 * dbgIn[tid][v].lights.size());
          if (which == 3) out.plain = -7;
          debug_calls(dbgIn[tid][v], &out, which);
          if (std::memcmp(&out, &dbgRef[tid][v], sizeof(out)) != 0) {
            static const char *names[] = {"rm_debug_ray_planes", "rm_debug_cull_bounds", "rm_debug_light_prep", "rm_debug_bulb_plain"};
            fail(tid, std::string(names[which]) + " differs from the serial result, call " + std::to_string(c));
            break;
          }
        }
      }

      // 3. the image readers
      barrier.wait();
      stamp(tid, 2);
      // every image is decoded by two threads (tid and tid + 4), beside six threads that decode other files
      for (size_t i = (size_t)tid % 4; i < images.size(); i += 4)
        if (image_record(images[i], (int)(i & 1)) != imageRef[i]) fail(tid, "image differs from the serial decode: " + images[i]);

      // 4. rm_last_error: odd threads provoke refusals with texts of their own, even threads only succeed
      uint8_t *px = nullptr;
      int w = 0, h = 0;
      const std::string mine = "/nonexistent/host_threads_" + std::to_string(tid) + ".png";
      if (rm_image_load(mine.c_str(), 0, &px, &w, &h) != RM_ERR_IO) fail(tid, "a missing image file was not RM_ERR_IO");
      const std::string before = rm_last_error();
      if (before != "could not open " + mine) fail(tid, "unexpected refusal text: " + before);
      RmCameraData good;
      std::memset(&good, 0, sizeof(good));
      good.pos[2] = 4.0f; good.pos[3] = 1.0f; good.look[2] = -1.0f; good.up[1] = 1.0f; good.heightAngle = 0.5f;
      barrier.wait();
      stamp(tid, 3);
      if (tid & 1) {
        RmCamera cam;
        RmObject obj;
        for (int c = 0; c < kErrorCalls; c++) {
          std::string want;
          int st;
          switch (c % 4) {
            case 0: {
              const std::string p = "/nonexistent/t" + std::to_string(tid) + "_" + std::to_string(c) + ".png";
              st = rm_image_load(p.c_str(), 0, &px, &w, &h);
              want = "could not open " + p;
              if (st != RM_ERR_IO) fail(tid, "a missing image file was not RM_ERR_IO");
              break;
            }
            case 1: st = rm_camera_build(nullptr, 4, 4, 0.1f, 100.0f, nullptr, nullptr, &cam); want = "bad camera arguments"; break;
            case 2: st = rm_camera_lens_samples(&good, 4, 4, 0.1f, 100.0f, 0.1f, 1.0f, 0, &cam); want = "lens samples: n must be at least 1"; break;
            default: st = rm_object_translated(nullptr, nullptr, &obj); want = "null argument"; break;
          }
          if (st == RM_OK) fail(tid, "a refusal returned RM_OK");
          const std::string got = rm_last_error();
          if (got != want) { fail(tid, "rm_last_error gave \"" + got + "\", this thread's last refusal was \"" + want + "\""); break; }
        }
      } else {
        DebugOutput out;
        for (int c = 0; c < kErrorCalls; c++) {
          const int v = c % kVar;
          RmCamera cam;
          if (rm_camera_build(&good, 64, 40, 0.1f, 100.0f, nullptr, nullptr, &cam) != RM_OK ||
              rm_debug_ray_planes(&dbgIn[tid][v].cam, out.planes) != RM_OK || rm_shard_rows(40, 8, 0, 2) < 0) {
            fail(tid, "a successful call failed");
            break;
          }
        }
        const std::string after = rm_last_error();
        if (after != before) fail(tid, "rm_last_error changed under successful calls: \"" + before + "\" became \"" + after + "\"");
      }
    });
  }
  for (auto &t : threads) t.join();
  stamp(0, 4);

  if (g_failures) { fprintf(stderr, "host_threads: %d failures\n", g_failures); return 1; }
  printf("host_threads: %d of %zu scenefiles loaded, %zu images, %d threads, %d calls of each rm_debug function per thread\n", loaded,
         scenes.size(), images.size(), kThreads, kDebugCalls);
  const auto ms = [](int a, int b) { return (int)std::chrono::duration_cast<std::chrono::milliseconds>(g_stamp[b] - g_stamp[a]).count(); };
  printf("host_threads: phases took %d ms (loader), %d ms (rm_debug_*), %d ms (images), %d ms (rm_last_error)\n", ms(0, 1), ms(1, 2), ms(2, 3), ms(3, 4));
  printf("host_threads ok\n");
  return 0;
}
