// The plain-C++ part of the column-engine layer (midagma_amd/csrc/coltest.h) on the CPU: the shape
// check, the column lists and the permutation count.  Built and run by tests/test_coltest_layer.py
// with -fsanitize=address,undefined; no HIP header is read.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "coltest.h"

using namespace midagma;

namespace {

int g_fail = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

bool is(const char* got, const char* want) { return got && want ? std::strcmp(got, want) == 0 : got == want; }

void shapes() {
  const double x = 0.0;
  CHECK(is(bad_shape(nullptr, 5, 3, 3), "null pointer"));
  CHECK(is(bad_shape(&x, 1, 3, 3), "need 2 <= n < 2^31 rows"));
  CHECK(is(bad_shape(&x, kMaxN + 1, 3, 3), "need 2 <= n < 2^31 rows"));
  CHECK(is(bad_shape(&x, 100, 3, 3, 99), "need 2 <= n < 2^31 rows"));  // a handle's own cap
  CHECK(is(bad_shape(&x, 5, 0, 3), "need 1 <= d <= 65535 columns"));
  CHECK(is(bad_shape(&x, 5, kMaxD + 1, kMaxD + 1), "need 1 <= d <= 65535 columns"));
  CHECK(is(bad_shape(&x, 5, 3, 2), "the leading dimension is below d"));
  // the first failing check names the reason
  CHECK(is(bad_shape(nullptr, 0, 0, -1), "null pointer") && is(bad_shape(&x, 0, 0, -1), "need 2 <= n < 2^31 rows"));
  CHECK(bad_shape(&x, 2, 1, 1) == nullptr && bad_shape(&x, kMaxN, kMaxD, kMaxD + 7) == nullptr);
  CHECK(bad_shape(&x, 99, 3, 3, 99) == nullptr);
}

using List = std::vector<int64_t>;

void column_lists() {
  for (int64_t d : {int64_t(1), int64_t(5)}) {
    List all, got{77};
    for (int64_t v = 0; v < d; ++v) all.push_back(v);
    // null: every column, whatever ncols says
    CHECK(listed_columns(nullptr, 0, d, got) == nullptr && got == all);
    CHECK(listed_columns(nullptr, -3, d, got) == nullptr && got == all);
    // empty
    const int64_t none = 0;
    CHECK(listed_columns(&none, 0, d, got) == nullptr && got.empty());
    // a negative count of a list that is there
    got = {77};
    CHECK(is(listed_columns(&none, -1, d, got), "ncols < 0") && got.empty());
    // duplicates and descending order: each once, ascending
    const List dup{d - 1, 0, d - 1, 0, 0};
    CHECK(listed_columns(dup.data(), (int64_t)dup.size(), d, got) == nullptr);
    CHECK(got == (d == 1 ? List{0} : List{0, d - 1}));
    List desc(all.rbegin(), all.rend());
    CHECK(listed_columns(desc.data(), d, d, got) == nullptr && got == all);
    // out of range, on either side, wherever it stands; nothing is listed
    for (int64_t bad : {int64_t(-1), d, d + 100}) {
      const List l{0, bad, 0};
      CHECK(is(listed_columns(l.data(), 3, d, got), "column index outside [0, d)") && got.empty());
      CHECK(is(listed_columns(l.data() + 1, 1, d, got), "column index outside [0, d)"));
      CHECK(listed_columns(l.data(), 1, d, got) == nullptr && got == List{0});  // (the bad one is not read)
    }
  }
  List got;
  const List some{3, 1, 3};
  CHECK(listed_columns(some.data(), 3, 5, got) == nullptr && got == (List{1, 3}));
}

// One evaluation of a run: pair q, permutation p (0: observed), the value the device left, whether
// the pair has a zero-range column.
struct Eval {
  int64_t q, p;
  double v;
  bool zero;
};

struct Counts {
  std::vector<double> stat, null;
  std::vector<int64_t> ge;
  Counts(int64_t m, int64_t P) : stat(m, -1.0), null(m * P, -1.0), ge(m, -1) {}
  bool operator==(const Counts& o) const { return stat == o.stat && null == o.null && ge == o.ge; }
};

// dcor_run's host loop as it stood before the layer: counted by the raw value, reported transformed
// (here sqrt(max(v, 0)); 0 for a zero-range pair)
void dcor_loop(const std::vector<Eval>& ev, int64_t P, double* stat, int64_t* ge, double* null_out) {
  double obs = 0.0;
  for (const Eval& e : ev) {
    const double s = e.zero ? 0.0 : std::sqrt(e.v > 0.0 ? e.v : 0.0);
    if (e.p == 0) {
      obs = e.v;
      stat[e.q] = s;
      ge[e.q] = e.zero ? P : 0;
    } else {
      if (!e.zero && e.v >= obs) ++ge[e.q];
      if (null_out) null_out[e.q * P + e.p - 1] = s;
    }
  }
}

// hsic_run's: a zero-range pair's value is 0, and what is counted is what is reported
void hsic_loop(const std::vector<Eval>& ev, int64_t P, double* stat, int64_t* ge, double* null_out) {
  double obs = 0.0;
  for (const Eval& e : ev) {
    const double v = e.zero ? 0.0 : e.v;
    if (e.p == 0) {
      obs = v;
      stat[e.q] = v;
      ge[e.q] = e.zero ? P : 0;
    } else {
      if (!e.zero && v >= obs) ++ge[e.q];
      if (null_out) null_out[e.q * P + e.p - 1] = v;
    }
  }
}

void permutation_counts() {
  // per pair: the observed value, then the permuted ones (P = 3 uses all, P = 1 the first): a tie
  // with the observed value, one above, one below; a negative observed value (dCor reports 0 and
  // still counts by the raw one); a zero-range pair, whose values are whatever the device left
  const double vals[4][4] = {{0.25, 0.25, 0.5, 0.125}, {-1e-3, -2e-3, -1e-3, 4.0}, {9.0, 10.0, 9.0, 8.0}, {1.0, 0.5, 2.0, 1.0}};
  const bool zero[4] = {false, false, true, false};
  for (int64_t P : {int64_t(0), int64_t(1), int64_t(3)}) {
    std::vector<Eval> ev;
    for (int64_t q = 0; q < 4; ++q)
      for (int64_t p = 0; p <= P; ++p) ev.push_back(Eval{q, p, vals[q][p], zero[q]});
    for (bool with_null : {true, false}) {
      Counts want_d(4, P), want_h(4, P), got_d(4, P), got_h(4, P);
      dcor_loop(ev, P, want_d.stat.data(), want_d.ge.data(), with_null ? want_d.null.data() : nullptr);
      hsic_loop(ev, P, want_h.stat.data(), want_h.ge.data(), with_null ? want_h.null.data() : nullptr);
      NullCount cd{got_d.stat.data(), got_d.ge.data(), with_null ? got_d.null.data() : nullptr, P};
      NullCount ch{got_h.stat.data(), got_h.ge.data(), with_null ? got_h.null.data() : nullptr, P};
      for (const Eval& e : ev) {
        cd.add(e.q, e.p, e.v, e.zero ? 0.0 : std::sqrt(e.v > 0.0 ? e.v : 0.0), e.zero);
        const double v = e.zero ? 0.0 : e.v;
        ch.add(e.q, e.p, v, v, e.zero);
      }
      CHECK(got_d == want_d && got_h == want_h);
      // the counts by hand: a tie counts, a zero-range pair counts every permutation
      const int64_t ge_d[3][4] = {{0, 0, 0, 0}, {1, 0, 1, 0}, {2, 2, 3, 2}};
      const int k = P == 0 ? 0 : P == 1 ? 1 : 2;
      for (int q = 0; q < 4; ++q) CHECK(got_d.ge[q] == ge_d[k][q] && got_h.ge[q] == ge_d[k][q]);
      CHECK(got_d.stat[0] == 0.5 && got_h.stat[0] == 0.25 && got_d.stat[1] == 0.0 && got_h.stat[1] == -1e-3);
      CHECK(got_d.stat[2] == 0.0 && got_h.stat[2] == 0.0);
      if (P == 3) {
        CHECK(got_d.null[2] == (with_null ? std::sqrt(0.125) : -1.0));  // (a null null_out is not written)
        CHECK(got_h.null[3 * 2 + 1] == (with_null ? 0.0 : -1.0));
      }
    }
  }
}

}  // namespace

int main() {
  shapes();
  column_lists();
  permutation_counts();
#if defined(__SANITIZE_ADDRESS__)
  std::printf("AddressSanitizer on\n");
#endif
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
