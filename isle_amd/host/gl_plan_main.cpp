// isle_amd/host/gl_plan_main.cpp — the host plan of the LDS-banded operator build (../csrc/gl_plan.h) for one case, as one JSON object on
// stdout: no library, no GPU (tests/test_gl_plan_cpu.py builds it with the address and undefined-behaviour sanitizers).
//   gl_plan_main <nnz> <D> <V> <cus> [g1=4..8] [g2=4..8] [rounds=0] [columns=0] [test_cus=N] [tot=zero|uniform|skew]
// The super-round totals the pass-2 schedule takes from the device (gl_blocktot_k) are made up here: all zero; 100 per (word block, document
// band); or rising from 100 in the first word block to 500 in the last (the blocks of a real corpus differ about five-fold).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/gl_plan.h"

namespace {

void put(const char* name, const std::vector<uint32_t>& v) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf(i ? ",%u" : "%u", v[i]);
  std::printf("]");
}
void put(const char* name, const std::vector<GlDesc>& v) {  // a descriptor as its eight words, in the struct's order
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i)
    std::printf("%s[%u,%u,%u,%u,%u,%u,%u,%u]", i ? "," : "", v[i].wave0, v[i].wstride, v[i].nw, v[i].b0, v[i].b1, v[i].slab, v[i].pos_base, v[i].pad);
  std::printf("]");
}
void put(const GlGeom& g) {
  std::printf("\"NB\": %u, \"nslice\": %u, \"nwv\": %u, \"wpg\": %u, \"G\": %d, ", g.NB, g.nslice, g.nwv, g.wpg, g.G);
  put("slice_of", g.slice_of);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: gl_plan_main <nnz> <D> <V> <cus> [g1=] [g2=] [rounds=0] [columns=0] [test_cus=] [tot=zero|uniform|skew]\n");
    return 2;
  }
  const uint64_t nnz = strtoull(argv[1], nullptr, 10);
  const uint32_t D = (uint32_t)strtoul(argv[2], nullptr, 10), V = (uint32_t)strtoul(argv[3], nullptr, 10), cus = (uint32_t)strtoul(argv[4], nullptr, 10);
  GlPlanOpts o;
  const char* totkind = "uniform";
  for (int i = 5; i < argc; ++i) {
    const char* eq = std::strchr(argv[i], '=');
    const size_t nk = eq ? (size_t)(eq - argv[i]) : 0;
    const auto is = [&](const char* k) { return nk == std::strlen(k) && !std::strncmp(argv[i], k, nk); };
    if (is("g1")) o.g1 = gl_forced_g(atoi(eq + 1));
    else if (is("g2")) o.g2 = gl_forced_g(atoi(eq + 1));
    else if (is("rounds")) o.rounds = atoi(eq + 1) != 0;
    else if (is("columns")) o.columns = atoi(eq + 1) != 0;
    else if (is("test_cus")) o.test_cus = (uint32_t)std::max(1, atoi(eq + 1));
    else if (is("tot")) totkind = eq + 1;
    else {
      std::fprintf(stderr, "gl_plan_main: unknown argument %s\n", argv[i]);
      return 2;
    }
  }
  if (!D || !V || !cus || (std::strcmp(totkind, "zero") && std::strcmp(totkind, "uniform") && std::strcmp(totkind, "skew"))) {
    std::fprintf(stderr, "gl_plan_main: D, V and cus must be positive, tot one of zero, uniform, skew\n");
    return 2;
  }
  const GlPlan1 p1 = gl_plan_pass1(nnz, D, V, cus, o);
  const GlGeom2 g2 = gl_plan_pass2_geometry(D, V, cus, o);
  const bool columns = gl_use_columns(g2.NB, o);
  const uint32_t per = columns ? g2.NB : 1u;  // totals per word block: one per band with columns, else the sum over the bands
  std::vector<unsigned long long> tot((size_t)g2.nblk * per);
  for (uint32_t ob = 0; ob < g2.nblk; ++ob) {
    const unsigned long long band = !std::strcmp(totkind, "zero") ? 0ull : !std::strcmp(totkind, "uniform") || g2.nblk < 2 ? 100ull : 100ull + 400ull * ob / (g2.nblk - 1);
    for (uint32_t z = 0; z < per; ++z) tot[(size_t)ob * per + z] = columns ? band : band * g2.NB;
  }
  const GlSched2 s = gl_plan_pass2_schedule(tot, g2.nblk, g2.NB, g2.wpg, g2.bitems, cus, columns);
  std::printf("{\"GL_RB\": %u, \"GL_NONE\": %u, \"pass1\": {", GL_RB, GL_NONE);
  put(p1);
  std::printf(", \"adjacent\": %s, ", p1.adjacent ? "true" : "false");
  put("desc", p1.desc);
  std::printf("}, \"pass2\": {");
  put(g2);
  std::printf(", \"nblk\": %u, \"bitems\": %u, \"columns\": %s, \"error\": %s%s%s, \"nslab\": %u, ", g2.nblk, g2.bitems, s.columns ? "true" : "false",
              s.error ? "\"" : "", s.error ? s.error : "null", s.error ? "\"" : "", s.nslab);
  put("cut", s.cut);
  std::printf(", ");
  put("slab0", s.slab0);
  std::printf(", ");
  put("nch", s.nch);
  std::printf(", ");
  put("desc", s.desc);
  std::printf("}}\n");
  return 0;
}
