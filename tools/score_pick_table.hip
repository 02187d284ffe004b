// The scoring selection table as text: pick_logpdf's answer for every bucket, variant code and `fast`, to compare two
// builds of the library (profiles/score_pick/).  Host only: it launches nothing and allocates nothing on a device.
//   hipcc -std=c++17 -I hpbandster_amd/csrc -I include tools/score_pick_table.hip -o score_pick_table \
//         -L hpbandster_amd/_lib -lhbx -Wl,-rpath,$PWD/hpbandster_amd/_lib -ldl
// Output: one line per distinct answer (the ScoreFns fields, kernels as numbers) with the combinations of (dc_pad,
// du_pad, variant, fast) that give it; then the numbered kernels, in order of first appearance, by the symbol name
// dladdr gives for the pointer ("?" if none: the numbers alone still show equal and unequal choices).
#include <cxxabi.h>
#include <dlfcn.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "hbx.h"
#include "hbx_score.h"

static std::vector<const void*> seen;

static int id_of(const void* p) {  // 0: null
  if (!p) return 0;
  for (size_t i = 0; i < seen.size(); ++i)
    if (seen[i] == p) return (int)i + 1;
  seen.push_back(p);
  return (int)seen.size();
}

static std::string name_of(const void* p) {
  Dl_info di;
  if (!dladdr(p, &di) || !di.dli_sname) return "?";
  int st = 0;
  char* d = abi::__cxa_demangle(di.dli_sname, nullptr, nullptr, &st);
  std::string s = (st == 0 && d) ? d : di.dli_sname;
  free(d);
  const size_t a = s.find("(double const*");  // every scoring kernel's first parameter: drop the signature
  if (a != std::string::npos) s.resize(a);
  if (di.dli_saddr != p) s += " +" + std::to_string((const char*)p - (const char*)di.dli_saddr);
  return s;
}

int main() {
  // every bucket hbx_kde_bucket can produce, and a few pairs that are none
  std::vector<std::pair<int, int>> dims;
  for (int dc = 0; dc <= 64; ++dc)
    for (int du = 0; du <= 32; ++du) {
      int32_t a, b, stride;
      if (hbx_kde_bucket(dc, du, &a, &b, &stride) != HBX_OK) continue;
      bool have = false;
      for (auto& d : dims) have = have || (d.first == a && d.second == b);
      if (!have) dims.push_back({a, b});
    }
  const size_t nbuckets = dims.size();
  for (auto d : {std::pair<int, int>{-1, -1}, {3, 0}, {8, 5}, {12, 4}, {40, 8}, {64, 64}, {128, 0}}) dims.push_back(d);
  // every variant code kde_params_kernel can emit (hbx_prep.hip prep_variant): hmode 0, the 16x16 tiles, the 32x32
  // tiles without and with a coarse table; signed or not; kc 0 to 4; exact_only where no table is built (hmode 0).
  // small_codes does not reach pick_logpdf.
  std::vector<int> variants;
  const int modes[4][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {1, 1, 1}};  // hmode, h32, coarse
  for (auto& m : modes)
    for (int neg = 0; neg < 2; ++neg)
      for (int kc = 0; kc <= 4; ++kc)
        for (int eo = 0; eo < (m[0] ? 1 : 2); ++eo) variants.push_back(KdeVariant{neg, kc, m[0], eo, m[1], m[2], 0}.encode());
  // the walk, in order: combination i = (index into dims * variants + index into variants) * 2 + fast
  printf("# dims (dc_pad,du_pad; the first %zu are the buckets):", nbuckets);
  for (auto& d : dims) printf(" %d,%d", d.first, d.second);
  printf("\n# variants:");
  for (int v : variants) printf(" %d", v);
  printf("\n# answer = main rescue cands_per_block threads pair rescue_pair split_ok pair1 list main_co : the combinations\n");
  std::vector<std::string> answers;            // distinct, in order of first appearance
  std::vector<std::vector<int>> where;         // ... and the combinations that give each
  int i = 0;
  for (auto& d : dims)
    for (int v : variants)
      for (int fast = 0; fast < 2; ++fast, ++i) {
        const ScoreFns f = pick_logpdf(d.first, d.second, v, fast != 0);
        char buf[160];
        snprintf(buf, sizeof buf, "%d %d %d %d %d %d %d %d %d %d", id_of((const void*)f.main),
                 id_of((const void*)f.rescue), f.cands_per_block, f.threads, id_of((const void*)f.pair),
                 id_of((const void*)f.rescue_pair), (int)f.split_ok, id_of((const void*)f.pair1),
                 id_of((const void*)f.list), id_of((const void*)f.main_co));
        size_t k = 0;
        while (k < answers.size() && answers[k] != buf) ++k;
        if (k == answers.size()) answers.push_back(buf), where.emplace_back();
        where[k].push_back(i);
      }
  for (size_t k = 0; k < answers.size(); ++k) {
    printf("%s :", answers[k].c_str());
    for (size_t a = 0; a < where[k].size();) {  // runs of consecutive combinations as first-last
      size_t b = a;
      while (b + 1 < where[k].size() && where[k][b + 1] == where[k][b] + 1) ++b;
      if (b > a) printf(" %d-%d", where[k][a], where[k][b]);
      else printf(" %d", where[k][a]);
      a = b + 1;
    }
    printf("\n");
  }
  printf("# kernels\n");
  for (size_t k = 0; k < seen.size(); ++k)  // four to a line
    printf("%zu %s%s", k + 1, name_of(seen[k]).c_str(), (k % 4 == 3 || k + 1 == seen.size()) ? "\n" : " | ");
  return 0;
}
