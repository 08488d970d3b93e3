// Host check of the workspace walker (ws.h) and of the layout functions of remd.hip, swap.hip and
// wct.hip, meant to be built with the host side under AddressSanitizer and UBSan
// (`make -C arbitrarystyletransfer_amd/csrc ws_check`); it launches nothing and needs no GPU. Each
// layout is walked over a heap block of exactly its `bytes`; every region is then written over the
// full extent that the launches use (stated here on its own, in the kernels' terms), so a region that
// is too short or a walk that ends past `bytes` is a sanitizer report; the regions must also be
// 256-byte aligned, disjoint, in order, and end at `bytes`. The stage layouts that share a compound
// op's scratch region are checked one stage at a time inside it. The three sources are included
// whole, each in a namespace of its own, so the layout functions under test are the library's, not
// copies.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/ast_hip.h"
#include "../../arbitrarystyletransfer_amd/csrc/det.h"
#include "../../arbitrarystyletransfer_amd/csrc/match_tile.h"
#include "../../arbitrarystyletransfer_amd/csrc/wave.h"
#include "../../arbitrarystyletransfer_amd/csrc/ws.h"

namespace remd_tu {
#include "../../arbitrarystyletransfer_amd/csrc/remd.hip"
}
namespace swap_tu {
#include "../../arbitrarystyletransfer_amd/csrc/swap.hip"
}
namespace wct_tu {
#include "../../arbitrarystyletransfer_amd/csrc/wct.hip"
}

namespace {

struct Region {
  const char* name;
  const void* p;
  int64_t bytes;  // what the launches read or write there
};

int failures = 0;

void fail(const char* what, const char* name, long long a, long long b) {
  printf("FAIL %s: %s (%lld, %lld)\n", what, name, a, b);
  ++failures;
}

// `regions` in walk order inside [base, base + total); `exact`: the last one ends at total
void check(const char* what, unsigned char* base, int64_t total, const std::vector<Region>& regions, bool exact) {
  int64_t end = 0;
  int id = 1;
  for (const Region& r : regions) {
    if (!r.p) {
      fail(what, r.name, -1, -1);
      continue;
    }
    const int64_t off = (const unsigned char*)r.p - base;
    if (off & 255) fail(what, r.name, off, 256);        // aligned
    if (off < end) fail(what, r.name, off, end);        // disjoint, in order
    if (off + r.bytes > total) fail(what, r.name, off + r.bytes, total);
    else memset(base + off, id++, (size_t)r.bytes);     // the sanitizer's view of the same bound
    end = ast_ws::al256(off + r.bytes);
  }
  if (exact ? end != total : end > total) fail(what, "end", end, total);
}

struct Block {
  unsigned char* p;
  int64_t bytes;
  explicit Block(int64_t b) : p((unsigned char*)malloc((size_t)(b > 0 ? b : 1))), bytes(b) {}
  ~Block() { free(p); }
};

void check_walk() {
  ast_ws::Walk null_walk(nullptr);
  if (null_walk.take<float>(1) || null_walk.take<int>(256) || null_walk.take<char>(257)) fail("walk", "null base", 0, 0);
  if (null_walk.off != 256 + 256 + 512) fail("walk", "offsets", null_walk.off, 1024);
  Block b(1024);
  ast_ws::Walk wk(b.p);
  check("walk", b.p, 1024, {{"a", wk.take<float>(1), 1}, {"b", wk.take<int>(256), 256}, {"c", wk.take<char>(257), 257}},
        true);
}

void check_remd(int n, int m, int p, int want) {
  using namespace remd_tu;
  const int64_t bytes = match_ws(nullptr, n, m, p, want).bytes;
  if (bytes != ast_cosine_match_workspace_bytes(n, n, m, p, want)) fail("remd", "query", bytes, 0);
  Block b(bytes);
  const MatchWs w = match_ws(b.p, n, m, p, want);
  const int64_t col = (int64_t)4 * n * ((m + 63) / 64) * p, row = (int64_t)4 * n * w.splits * m;
  std::vector<Region> r = {{"pcol", w.pcol, col}, {"pcidx", w.pcidx, col}};
  if (w.splits > 1) r.insert(r.end(), {{"prow", w.prow, row}, {"pridx", w.pridx, row}});
  else if (w.prow || w.pridx) fail("remd", "row partials of one split", 0, 0);
  check("remd match", b.p, bytes, r, true);

  const int64_t bb = bwd_ws(nullptr, n, m, p).bytes;
  Block g(bb);
  const BwdWs v = bwd_ws(g.p, n, m, p);
  check("remd backward", g.p, bb,
        {{"start", v.start, (int64_t)4 * n * (m + 1)}, {"cursor", v.cursor, (int64_t)4 * n * m}, {"list", v.list, (int64_t)4 * n * p}},
        true);
}

std::vector<Region> swap_match_regions(const swap_tu::MatchWs& w, int n, int S, int64_t m, int64_t ns) {
  const int64_t ct = (m + 63) / 64, bt = (ns + 63) / 64;
  std::vector<Region> r = {{"score", w.score, 4 * n * m}};
  if (S > 0) r.insert(r.end(), {{"cmask", w.cmask, 8 * n * ct}, {"bmask", w.bmask, 8 * S * bt}});
  if (w.splits > 1) r.insert(r.end(), {{"pscore", w.pscore, 4 * n * w.splits * m}, {"pindex", w.pindex, 4 * n * w.splits * m}});
  return r;
}

// S = 0: the unguided op with ns style maps; S > 0: a bank of S styles
void check_swap(int n, int ns, int S, int hc, int wc, int hs, int ws, int want) {
  using namespace swap_tu;
  const int64_t m = (int64_t)(hc - 2) * (wc - 2), sp = (int64_t)(hs - 2) * (ws - 2);
  const int64_t mb = match_ws(nullptr, n, S, hc, wc, hs, ws, want).bytes;
  Block b(mb);
  check("swap match", b.p, mb, swap_match_regions(match_ws(b.p, n, S, hc, wc, hs, ws, want), n, S, m, sp), true);

  const int64_t bytes = swap_ws(nullptr, n, ns, S, hc, wc, hs, ws).bytes;
  const long long q = S > 0 ? ast_style_swap_guided_workspace_bytes(n, S, hc, wc, hs, ws)
                            : ast_style_swap_workspace_bytes(n, ns, hc, wc, hs, ws);
  if (bytes != q) fail("swap", "query", bytes, q);
  Block g(bytes);
  const SwapWs w = swap_ws(g.p, n, ns, S, hc, wc, hs, ws);
  // the scratch: the norms' pixels and the match's regions start together and both fit
  unsigned char* scratch = (unsigned char*)w.scratch;
  check("swap", g.p, bytes, {{"inv", w.inv, 4 * ns * sp}, {"index", w.index, 4 * n * m}, {"norms", scratch, (int64_t)4 * ns * hs * ws}},
        false);
  const MatchWs mw = match_ws(scratch, n, S, hc, wc, hs, ws, 0);
  check("swap scratch", scratch, bytes - (scratch - g.p), swap_match_regions(mw, n, S, m, sp), false);
  const int64_t used = norms_ws(ns, hs, ws) > mw.bytes ? norms_ws(ns, hs, ws) : mw.bytes;
  if ((scratch - g.p) + used != bytes) fail("swap", "end", (scratch - g.p) + used, bytes);
}

std::vector<Region> sqrt_regions(const wct_tu::SqrtWs& s, int b, int c) {
  const int64_t two = (int64_t)4 * 2 * b * c * c;  // Y then Z, b matrices each
  return {{"norm", s.norm, (int64_t)4 * b}, {"yz0", s.yz[0], two}, {"yz1", s.yz[1], two}, {"P", s.P, two / 2}};
}

std::vector<Region> mix_regions(const wct_tu::RegionMixWs& s, int n, int c, int k) {
  const int64_t nk = (int64_t)n * k;
  return {{"valid", s.valid, 4 * nk}, {"mmix", s.mmix, 4 * nk * c}, {"cmix", s.cmix, 4 * nk * c * c}, {"T", s.T, 4 * nk * c * c}};
}

int64_t part_floats(int matrices, int c, int slots) {
  const int64_t t = (c + 63) / 64;
  return (int64_t)matrices * slots * (t * (t + 1) / 2) * 64 * 64;
}

void check_wct(int n, int ns, int c, int64_t mc, int64_t ms) {
  using namespace wct_tu;
  const int b = n + ns;
  const int64_t bytes = wct_ws(nullptr, n, ns, c, mc, ms).bytes;
  if (bytes != ast_wct_workspace_bytes(n, ns, c, mc, ms)) fail("wct", "query", bytes, 0);
  Block g(bytes);
  const WctWs w = wct_ws(g.p, n, ns, c, mc, ms);
  const int64_t vec = (int64_t)4 * b * c, mat = vec * c;
  unsigned char* scratch = (unsigned char*)w.scratch;
  const int64_t left = bytes - (scratch - g.p);
  check("wct", g.p, bytes, {{"mean", w.mat.mean, vec}, {"cov", w.mat.cov, mat}, {"root", w.mat.root, mat}, {"iroot", w.mat.iroot, mat},
                            {"scratch", scratch, left}}, true);
  check("wct content partials", scratch, left, {{"part", scratch, 4 * part_floats(n, c, cov_splits(mc, nullptr))}}, false);
  check("wct style partials", scratch, left, {{"part", scratch, 4 * part_floats(ns, c, cov_splits(ms, nullptr))}}, false);
  check("wct sqrt", scratch, left, sqrt_regions(sqrt_ws(scratch, b, c), b, c), false);
  check("wct apply", scratch, left, {{"T", scratch, (int64_t)4 * n * c * c}}, false);
}

void check_wct_regions(int n, int c, int64_t mc, int k, int s, int64_t ms, int reg) {
  using namespace wct_tu;
  const int b = n * k + s * (reg ? k : 1);
  const int64_t bytes = regions_ws(nullptr, n, c, mc, k, s, ms, reg).bytes;
  Block g(bytes);
  const RegionsWs w = regions_ws(g.p, n, c, mc, k, s, ms, reg);
  const int64_t vec = (int64_t)4 * b * c, mat = vec * c;
  unsigned char* scratch = (unsigned char*)w.scratch;
  const int64_t left = bytes - (scratch - g.p);
  check("wct regions", g.p, bytes,
        {{"mean", w.mat.mean, vec}, {"cov", w.mat.cov, mat}, {"root", w.mat.root, mat}, {"iroot", w.mat.iroot, mat},
         {"cperm", w.cperm, 4 * n * mc}, {"ccount", w.ccount, (int64_t)4 * n * k}, {"sperm", w.sperm, 4 * s * ms},
         {"scount", w.scount, (int64_t)4 * s * k}, {"scratch", scratch, left}}, true);
  check("wct regions content partials", scratch, left, {{"part", scratch, 4 * part_floats(n * k, c, region_slots(mc))}}, false);
  const int64_t sp = reg ? part_floats(s * k, c, region_slots(ms)) : part_floats(s, c, cov_splits(ms, nullptr));
  check("wct regions style partials", scratch, left, {{"part", scratch, 4 * sp}}, false);
  check("wct regions sqrt", scratch, left, sqrt_regions(sqrt_ws(scratch, b, c), b, c), false);
  check("wct regions mix", scratch, left, mix_regions(region_mix_ws(scratch, n, c, k), n, c, k), false);

  const int64_t ab = region_apply_ws(nullptr, n, c, mc, k).bytes;
  Block a(ab);
  const RegionApplyWs v = region_apply_ws(a.p, n, c, mc, k);
  std::vector<Region> r = {{"perm", v.perm, 4 * n * mc}, {"count", v.count, (int64_t)4 * n * k}};
  const std::vector<Region> mx = mix_regions(region_mix_ws(v.mix, n, c, k), n, c, k);
  r.insert(r.end(), mx.begin(), mx.end());
  check("wct region apply", a.p, ab, r, true);
}

}  // namespace

int main() {
  check_walk();
  for (int want : {0, 1, 3}) {
    check_remd(2, 70, 130, want);
    check_remd(16, 1024, 1024, want);
    check_swap(2, 1, 0, 12, 12, 14, 14, want);
    check_swap(2, 2, 2, 12, 12, 14, 14, want);
  }
  check_swap(1, 1, 0, 64, 64, 64, 64, 0);
  check_swap(128, 3, 3, 12, 12, 64, 64, 0);  // the norms' scratch is the larger one
  check_wct(2, 1, 72, 99, 63);
  check_wct(2, 2, 72, 448, 449);
  check_wct(8, 1, 3, 65536, 513);            // the covariance partials are the largest stage
  for (int reg : {0, 1}) {
    check_wct_regions(2, 72, 99, 3, 2, 63, reg);
    check_wct_regions(1, 64, 512, 8, 3, 513, reg);
  }
  printf(failures ? "ws_check: %d failures\n" : "ws_check: ok\n", failures);
  return failures ? 1 : 0;
}
