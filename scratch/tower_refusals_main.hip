// Host-only refusals of the ViT tower under a sanitizer; needs no device (every call below returns before any HIP call):
//   cd ovmono3d_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       ../../scratch/tower_refusals_main.hip tower.hip loader.hip -I. -L.. -lovm3d -Wl,-rpath,$PWD/.. -o /tmp/tower_refusals && /tmp/tower_refusals
// (libovm3d.so only supplies the kernel launchers tower.hip names; the tower and the loader are the sanitized objects.)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "tower.hpp"

using namespace ovm;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static TowerConfig good(int family) {
  TowerConfig c; std::memset(&c, 0, sizeof(c));
  c.family = family; c.embed_dim = 128; c.depth = 2; c.heads = 2; c.pos_grid = 4; c.precision = 3; c.max_batch = 1;
  c.canvas = kFamilies[family].patch * 4; c.sam_window = 2;
  return c;
}

struct Table {                       // an OvmTensor table over buffers of exactly the stated size (a read past one is a sanitizer error)
  std::vector<std::vector<float>> data; std::vector<std::string> names; std::vector<OvmTensor> t;
  void add(const std::string& name, std::vector<int64_t> shape) {
    int64_t n = 1; for (int64_t s : shape) n *= s;
    data.emplace_back((size_t)n, 0.5f); names.push_back(name);
    OvmTensor x; std::memset(&x, 0, sizeof(x));
    x.ndim = (int)shape.size(); for (size_t i = 0; i < shape.size(); ++i) x.shape[i] = shape[i];
    t.push_back(x);
  }
  const OvmTensor* table() { for (size_t i = 0; i < t.size(); ++i) { t[i].name = names[i].c_str(); t[i].data = data[i].data(); } return t.data(); }
};

// configure + load of the hub family on a checkpoint that must be refused before the device is touched
static int hub_load(Table& tb, int precision, std::string* err) {
  Tower t; TowerConfig c = good(FAM_DINOV2_HUB); c.precision = precision;
  CHECK(t.configure(c) == OVM_OK);
  const int r = t.load(tb.table(), (int)tb.t.size(), 0);
  *err = t.err;
  return r;
}

int main() {
  // ---- every row: the geometry refusals of configure
  for (int f = 0; f < FAM_COUNT; ++f) {
    { Tower t; CHECK(t.configure(good(f)) == OVM_OK && t.fam == &kFamilies[f] && t.G == 4 && t.D == 128 && t.Kpe >= 3 * t.patch * t.patch); }
    { Tower t; TowerConfig c = good(f); c.canvas += 1; CHECK(t.configure(c) == OVM_ERR_INVALID && t.err == kErrTowerGeometry); }
    { Tower t; TowerConfig c = good(f); c.embed_dim = 384; c.heads = 6; CHECK(t.configure(c) == OVM_OK); }
    { Tower t; TowerConfig c = good(f); c.embed_dim = 64; c.heads = 1; CHECK(t.configure(c) == OVM_ERR_INVALID); }
    { Tower t; TowerConfig c = good(f); c.heads = 4; CHECK(t.configure(c) == OVM_ERR_INVALID); }
    { Tower t; TowerConfig c = good(f); c.precision = 2; CHECK(t.configure(c) == OVM_ERR_INVALID); }
    { Tower t; TowerConfig c = good(f); c.max_batch = 0; CHECK(t.configure(c) == OVM_ERR_INVALID && t.err == kErrTowerGeometry); }
    { Tower t; TowerConfig c = good(f); c.ln_eps = 1e-3f; CHECK(t.configure(c) == OVM_OK && t.ln_eps == 1e-3f); }
  }
  { Tower t; TowerConfig c = good(0); c.family = FAM_COUNT; CHECK(t.configure(c) == OVM_ERR_INVALID && t.err == "invalid config (tower)"); }
  { Tower t; TowerConfig c = good(0); c.family = -1; CHECK(t.configure(c) == OVM_ERR_INVALID && t.err == "invalid config (tower)"); }
  { Tower t; TowerConfig c = good(FAM_SAM); c.sam_window = 0; CHECK(t.configure(c) == OVM_ERR_INVALID && t.err == "invalid config (sam_window, depth <= 32, pos_grid)"); }
  { Tower t; TowerConfig c = good(FAM_SAM); c.depth = 33; CHECK(t.configure(c) == OVM_ERR_INVALID); }
  { Tower t; TowerConfig c = good(FAM_SAM); c.pos_grid = 0; CHECK(t.configure(c) == OVM_ERR_INVALID); }

  // ---- hub DINOv2: the checkpoint's variants, on short and mis-shaped tables
  const std::string V = "backbone.net.vit.", M0 = V + "blocks.0.mlp.";
  std::string e;
  { Table tb; tb.add(V + "register_tokens", {1, 4}); CHECK(hub_load(tb, 3, &e) == OVM_ERR_SHAPE && e == "bad shape for " + V + "register_tokens (expected [1][R][embed_dim])"); }
  { Table tb; tb.add(V + "register_tokens", {2, 4, 128}); CHECK(hub_load(tb, 3, &e) == OVM_ERR_SHAPE); }
  { Table tb; tb.add(V + "register_tokens", {1, 4, 64}); CHECK(hub_load(tb, 3, &e) == OVM_ERR_SHAPE); }
  { Table tb; tb.add(V + "register_tokens", {1, 17, 128}); CHECK(hub_load(tb, 3, &e) == OVM_ERR_CAPACITY && e == V + "register_tokens: more than 16 register tokens"); }
  { Table tb; tb.add(V + "register_tokens", {1, 4, 128});
    CHECK(hub_load(tb, 3, &e) == OVM_ERR_MISSING_WEIGHT && e == "missing weight: " + M0 + "fc1.weight or " + M0 + "w12.weight"); }
  { Table tb; tb.add(M0 + "w12.weight", {8, 128}); tb.add(M0 + "fc1.weight", {1});
    CHECK(hub_load(tb, 3, &e) == OVM_ERR_INVALID && e == "checkpoint has both " + M0 + "w12.weight and " + M0 + "fc1.weight"); }
  { Table tb; tb.add(M0 + "w12.weight", {7, 128}); CHECK(hub_load(tb, 3, &e) == OVM_ERR_SHAPE && e == "bad shape for " + M0 + "w12.weight (expected [2 Hs][embed_dim])"); }
  { Table tb; tb.add(M0 + "w12.weight", {8, 64}); CHECK(hub_load(tb, 3, &e) == OVM_ERR_SHAPE); }
  { Table tb; tb.add(M0 + "w12.weight", {1024}); CHECK(hub_load(tb, 3, &e) == OVM_ERR_SHAPE); }
  { Table tb; tb.add(M0 + "w12.weight", {8, 128}); CHECK(hub_load(tb, 3, &e) == OVM_ERR_MISSING_WEIGHT && e == "missing weight: " + M0 + "w3.weight"); }
  { Table tb; tb.add(M0 + "w12.weight", {8, 128}); tb.add(M0 + "w3.weight", {128, 5});
    CHECK(hub_load(tb, 3, &e) == OVM_ERR_SHAPE && e == "bad shape for " + M0 + "w3.weight (expected [embed_dim][4] after " + M0 + "w12.weight)"); }
  { Table tb; tb.add(M0 + "w12.weight", {8, 128}); tb.add(M0 + "w3.weight", {4, 128}); CHECK(hub_load(tb, 1, &e) == OVM_ERR_SHAPE); }
  for (int precision : {1, 3}) {                 // 4 D = 512: Hs = 512 fits exactly, 513 does not (padded to 544 / 576)
    Table tb; tb.add(M0 + "w12.weight", {1026, 128}); tb.add(M0 + "w3.weight", {128, 513});
    CHECK(hub_load(tb, precision, &e) == OVM_ERR_CAPACITY && e == M0 + "w12.weight: hidden width exceeds 4 * embed_dim");
  }

  // ---- the host helpers of the two files, on the smallest tables they take
  {
    const int D = 8, M = 3, G = 5;
    std::vector<float> pos((size_t)(1 + M * M) * D, 0.25f), out((size_t)(1 + G * G) * D), same((size_t)(1 + M * M) * D);
    CHECK(ovm_host_resize_pos_embed_aa(pos.data(), M, D, G, out.data()) == OVM_OK && ovm_host_resize_pos_embed_aa(pos.data(), M, D, M, same.data()) == OVM_OK);
    CHECK(ovm_host_interp_pos_embed(pos.data(), M, D, G, out.data()) == OVM_OK && ovm_host_interp_pos_embed(pos.data(), M, D, 1, out.data()) == OVM_OK);
    CHECK(ovm_host_resize_pos_embed_aa(pos.data(), 0, D, G, out.data()) == OVM_ERR_INVALID && ovm_host_interp_pos_embed(pos.data(), M, 0, G, out.data()) == OVM_ERR_INVALID);
    CHECK(ovm_host_sincos_pos_embed(D, G, out.data()) == OVM_OK && ovm_host_sincos_pos_embed(6, G, out.data()) == OVM_ERR_INVALID);
    std::vector<int32_t> perm(2 * 32);
    CHECK(ovm_host_swiglu_perm(17, perm.data()) == OVM_OK && ovm_host_swiglu_perm(0, perm.data()) == OVM_ERR_INVALID);
    std::vector<float> w(3 * 5, 1.f); std::vector<half_t> img(packed_halves(3, 32, 3));
    CHECK(host_pack_weight(w.data(), 3, 5, 32, 3, img.data()) == OVM_OK && host_pack_weight(w.data(), 3, 5, 8, 3, img.data()) == OVM_ERR_SHAPE);
    CHECK(host_pack_weight(w.data(), 3, 5, 4, 1, img.data()) == OVM_ERR_INVALID);
  }
  std::printf(fails ? "%d check(s) failed\n" : "tower host checks ok\n", fails);
  return fails != 0;
}
