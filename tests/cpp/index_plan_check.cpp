// Host-side check of needle_amd/csrc/index_plan.h, the incremental index's host plan, with nothing of ROCm on the include path.
//   1. Lists without labels against the expressions index.cpp had before the plan (namespace before, carried verbatim): every
//      (n0, k) with n0 + k <= 40, regions 1 and 2, min_len with zeros sprinkled in -- first_pair, new_pairs, searched, the
//      problem list element for element, the inverse of the id (the sqrt form), least[] on both routes.
//   2. Labelled lists (1 to 6 labels over up to 40 videos, interleaved, a label with one member, a label that first appears
//      among the arriving videos) against brute force over index_group_pair.
//   3. One label plans what no labels plan, field for field; only labelled() differs.
//   4. at(id(i, j)) == (i, j) for every pair of every list; the unlabelled list at the two sizes where pairs x regions
//      crosses 0xFFFFFFF0.
//   5. Appends compose: 0 -> n in one step lists what any split into steps lists, under the same absolute ids.
//   6. Edits against the loops index.cpp had and against brute force.
//   7. least[] against brute force on both routes (in 1 and 2), a region without a live pair included.
//   8. Acceptance: every fact flipped alone, and every adjacent pair of the chain flipped together, per route.
// Prints "index plan ok" and returns 0, or one line per broken invariant.
#include <cmath>
#include <cstdio>
#include <functional>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../needle_amd/csrc/index_plan.h"

using namespace needle;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)               \
  do {                                 \
    if (!(cond)) {                     \
      if (g_failed < 50) {             \
        std::printf("INVARIANT ");     \
        std::printf(__VA_ARGS__);      \
        std::printf(" (%s)\n", #cond); \
      }                                \
      g_failed++;                      \
    }                                  \
  } while (0)

bool same(const NeedleHipProblem &a, const NeedleHipProblem &b) {
  return a.src_seq == b.src_seq && a.dst_seq == b.dst_seq && a.min_len == b.min_len && a.tag == b.tag;
}
bool same(const std::vector<NeedleHipProblem> &a, const std::vector<NeedleHipProblem> &b) {
  if (a.size() != b.size()) return false;
  for (size_t q = 0; q < a.size(); q++)
    if (!same(a[q], b[q])) return false;
  return true;
}

// min_len of `rows` rows: 1 to 9, about a quarter zeros; dead: every row of region 1 is zero (no pair is live there)
std::vector<uint32_t> some_min_len(std::mt19937 &rng, size_t videos, size_t R, bool dead = false) {
  std::vector<uint32_t> m(videos * R);
  for (size_t at = 0; at < m.size(); at++) m[at] = rng() % 4 == 0 || (dead && at % R == 1) ? 0u : 1u + rng() % 9;
  return m;
}

// ---- what index.cpp computed before the plan, verbatim ---------------------------------------------------------------------
namespace before {

void column_pair(uint64_t p, size_t *pi, size_t *pj) {  // p(i, j) = j (j - 1) / 2 + i, inverted
  size_t j = (size_t)((1.0 + std::sqrt(1.0 + 8.0 * (double)p)) / 2.0);
  while (j > 1 && (uint64_t)j * (j - 1) / 2 > p) j--;
  while ((uint64_t)(j + 1) * j / 2 <= p) j++;
  *pi = (size_t)(p - (uint64_t)j * (j - 1) / 2);
  *pj = j;
}

bool pair_problems(const std::vector<uint32_t> &min_len, size_t R, size_t i, size_t j, uint64_t tag, std::vector<NeedleHipProblem> *problems) {
  bool any = false;
  for (size_t r = 0; r < R; r++) {
    const uint32_t a = min_len[i * R + r], b = min_len[j * R + r];
    if (a == 0 || b == 0) continue;
    problems->push_back(NeedleHipProblem{(uint32_t)(i * R + r), (uint32_t)(j * R + r), std::max(a, b), (uint32_t)(tag + r)});
    any = true;
  }
  return any;
}

struct Append {
  uint64_t first_pair = 0, new_pairs = 0, searched = 0;
  std::vector<NeedleHipProblem> problems;
};

// Index::append's pair arithmetic and its loops (groups null: the plain index)
Append append(size_t n0, size_t n1, size_t R, const std::vector<uint32_t> &min_len, const IndexGroupTables *groups) {
  Append out;
  const uint64_t all_pairs = groups ? groups->pairs() : (uint64_t)n1 * (n1 - 1) / 2;
  const uint64_t first_pair = groups ? groups->vbase[n0] : (uint64_t)n0 * (n0 ? n0 - 1 : 0) / 2;
  const uint64_t new_pairs = all_pairs - first_pair;
  std::vector<NeedleHipProblem> problems;
  uint64_t searched = 0;
  for (size_t j = n0; j < n1; j++) {
    if (groups) {
      const uint32_t *members = groups->members.data() + groups->first[groups->group_of[j]];
      for (size_t ra = 0; ra < groups->rank_of[j]; ra++)
        searched += pair_problems(min_len, R, members[ra], j, (groups->vbase[j] + ra - first_pair) * R, &problems);
      continue;
    }
    for (size_t i = 0; i < j; i++) searched += pair_problems(min_len, R, i, j, ((uint64_t)j * (j - 1) / 2 + i - first_pair) * R, &problems);
  }
  out.first_pair = first_pair;
  out.new_pairs = new_pairs;
  out.searched = searched;
  out.problems.swap(problems);
  return out;
}

// the bound of the matched route (streamed: the cross-matcher had the arriving pairs only)
uint32_t least(size_t n0, size_t n1, size_t R, size_t r, const std::vector<uint32_t> &min_len, const IndexGroupTables *groups, bool streamed) {
  uint32_t least = UINT32_MAX;
  for (size_t j = n0; j < n1; j++)
    for (size_t i = streamed ? n0 : 0; i < j; i++)
      if ((!groups || groups->group_of[i] == groups->group_of[j]) && min_len[i * R + r] && min_len[j * R + r])
        least = std::min(least, std::max(min_len[i * R + r], min_len[j * R + r]));
  return least;
}

struct Edit {
  std::vector<uint32_t> new_of_old, gone, pair_ids;
  std::vector<NeedleHipProblem> problems;
  std::vector<std::pair<size_t, size_t>> listed;
  uint64_t searched = 0;
};

constexpr uint32_t kIndexFresh = 0xFFFFFFFFu;

// Index::rebuild's tables and its listing loops
Edit edit(size_t n0, const std::vector<uint32_t> &old_of_new, size_t R, const std::vector<uint32_t> &min_len, const IndexGroupTables *groups) {
  Edit out;
  const size_t n1 = old_of_new.size();
  auto is_fresh = [&](size_t v) { return old_of_new[v] == kIndexFresh; };
  std::vector<uint32_t> new_of_old(n0, kIndexFresh), gone;
  for (size_t v = 0; v < n1; v++)
    if (!is_fresh(v)) new_of_old[old_of_new[v]] = (uint32_t)v;
  for (size_t q = 0; q < n0; q++)
    if (new_of_old[q] == kIndexFresh) gone.push_back((uint32_t)q);
  std::vector<uint32_t> pair_ids;
  std::vector<NeedleHipProblem> problems;
  uint64_t searched = 0;
  auto list_pair = [&](size_t i, size_t j) {
    out.listed.emplace_back(i, j);
    searched += pair_problems(min_len, R, i, j, (uint64_t)pair_ids.size() * R, &problems);
    pair_ids.push_back((uint32_t)(groups ? groups->vbase[j] + groups->rank_of[i] : (uint64_t)j * (j - 1) / 2 + i));
  };
  for (size_t f = 0; f < n1; f++) {
    if (!is_fresh(f)) continue;
    if (groups) {  // its pairs inside its group only
      const uint32_t g = groups->group_of[f];
      for (uint32_t m = 0; m < groups->size[g]; m++) {
        const size_t q = groups->members[groups->first[g] + m];
        if (q < f) list_pair(q, f);
        else if (q > f && !is_fresh(q)) list_pair(f, q);
      }
      continue;
    }
    for (size_t q = 0; q < f; q++) list_pair(q, f);
    for (size_t q = f + 1; q < n1; q++)
      if (!is_fresh(q)) list_pair(f, q);
  }
  out.new_of_old.swap(new_of_old);
  out.gone.swap(gone);
  out.pair_ids.swap(pair_ids);
  out.problems.swap(problems);
  out.searched = searched;
  return out;
}

}  // namespace before

bool g_saw_no_live_pair = false;

std::vector<uint32_t> listed(const IndexPairIds::Members &m) {
  std::vector<uint32_t> out;
  for (uint32_t v : m) out.push_back(v);
  return out;
}

// (4, and the interface of a.) every question IndexPairIds answers, against brute force over the labels (null: none)
void check_ids(const IndexPairIds &ids, const uint32_t *labels, size_t n, const char *what) {
  auto together = [&](size_t i, size_t j) { return !labels || labels[i] == labels[j]; };
  const std::vector<uint32_t> one(n, 0u);
  const IndexGroupTables tables(labels ? labels : one.data(), n);  // pair_ids.h's own, one label where there are none
  CHECK(ids.videos() == n && ids.labelled() == (labels != nullptr), "%s: n %zu", what, n);
  CHECK((ids.store_groups() != nullptr) == (labels != nullptr), "%s: the store's tables are null exactly for a plain list", what);
  CHECK(ids.column(n) == ids.pairs(), "%s: n %zu", what, n);
  std::set<uint64_t> seen;
  uint64_t pairs = 0;
  for (size_t j = 0; j < n; j++) {
    std::vector<uint32_t> lower, group;
    for (size_t i = 0; i < n; i++) {
      if (!together(i, j)) continue;
      group.push_back((uint32_t)i);
      if (i < j) lower.push_back((uint32_t)i);
    }
    CHECK(listed(ids.lower(j)) == lower, "%s: n %zu lower partners of %zu", what, n, j);
    CHECK(listed(ids.group(j)) == group, "%s: n %zu partners of %zu", what, n, j);
    CHECK(ids.paired(j) == (group.size() > 1), "%s: n %zu paired(%zu)", what, n, j);
    CHECK(ids.column(j + 1) - ids.column(j) == lower.size(), "%s: n %zu column of %zu", what, n, j);
    for (size_t q = 0; q < lower.size(); q++) {
      const size_t i = lower[q];
      const uint64_t id = ids.id(i, j);
      uint64_t want = 0;
      CHECK(index_group_pair(tables.view(), (uint32_t)i, (uint32_t)j, &want) && want == id, "%s: n %zu id(%zu, %zu)", what, n, i, j);
      CHECK(id == ids.column(j) + q, "%s: n %zu (%zu, %zu) is not at its place in the column", what, n, i, j);
      if (!labels) CHECK(id == column_major_pair(i, j), "%s: n %zu (%zu, %zu) is not the column-major id", what, n, i, j);
      size_t ai = ~(size_t)0, aj = ~(size_t)0;
      CHECK(ids.at(id, &ai, &aj) && ai == i && aj == j, "%s: n %zu at(id(%zu, %zu)) = (%zu, %zu)", what, n, i, j, ai, aj);
      CHECK(ids.together(i, j) && id < ids.pairs() && seen.insert(id).second, "%s: n %zu id %llu of (%zu, %zu)", what, n,
            (unsigned long long)id, i, j);
      pairs++;
    }
    for (size_t i = 0; i < j; i++) CHECK(ids.together(i, j) == together(i, j), "%s: n %zu together(%zu, %zu)", what, n, i, j);
  }
  size_t i = 0, j = 0;
  CHECK(ids.pairs() == pairs && !ids.at(pairs, &i, &j), "%s: n %zu pairs %llu", what, n, (unsigned long long)ids.pairs());
}

// the plan of one append, both stages, on `route`; min_len of all n1 x R rows
IndexAppendPlan planned(size_t n0, size_t k, size_t R, const uint32_t *labels, const std::vector<uint32_t> &min_len, IndexRoute route) {
  const std::vector<uint32_t> old_labels(labels, labels + (labels ? n0 : 0));
  IndexAppendPlan p = plan_index_append(n0, k, R, old_labels, labels ? labels + n0 : nullptr);
  CHECK(p.refusal.ok() && p.ids, "append %zu + %zu refused", n0, k);
  const IndexRefusal no = list_index_append(&p, min_len.data(), route);
  CHECK(no.ok(), "append %zu + %zu: %s", n0, k, no.text.c_str());
  return p;
}

// (1, 2, 7) one append against index.cpp's former loops and against brute force
void check_append(size_t n0, size_t k, size_t R, const uint32_t *labels, const std::vector<uint32_t> &min_len, const char *what) {
  const size_t n1 = n0 + k;
  std::unique_ptr<IndexGroupTables> groups(labels ? new IndexGroupTables(labels, n1) : nullptr);
  const before::Append want = before::append(n0, n1, R, min_len, groups.get());
  const IndexAppendPlan p = planned(n0, k, R, labels, min_len, IndexRoute::Matched);
  CHECK(p.n0 == n0 && p.n1 == n1 && p.regions == R, "%s %zu + %zu", what, n0, k);
  CHECK(p.first_pair == want.first_pair && p.new_pairs == want.new_pairs && p.searched == want.searched, "%s %zu + %zu x %zu: counts", what, n0, k, R);
  CHECK(same(p.problems, want.problems), "%s %zu + %zu x %zu: the problem list", what, n0, k, R);
  CHECK(p.labels == (labels ? std::vector<uint32_t>(labels, labels + n1) : std::vector<uint32_t>()), "%s %zu + %zu: labels", what, n0, k);
  if (!labels) {
    CHECK(p.first_pair == (n0 ? column_major_pair(0, n0) : 0) && p.first_pair + p.new_pairs == (uint64_t)n1 * (n1 - 1) / 2, "%s %zu + %zu", what, n0, k);
    for (uint64_t q = 0; q < p.new_pairs; q++) {
      size_t i = 0, j = 0, wi = 0, wj = 0;
      before::column_pair(p.first_pair + q, &wi, &wj);
      CHECK(p.ids->at(p.first_pair + q, &i, &j) && i == wi && j == wj, "%s %zu + %zu: at(%llu)", what, n0, k, (unsigned long long)(p.first_pair + q));
    }
  }
  // brute force: exactly the same-label pairs (i, j), j >= n0, i < j, in ascending id, tag (id - first) R + r
  const IndexGroupTables one(std::vector<uint32_t>(n1, 0u).data(), n1);
  const IndexGroupView view = labels ? groups->view() : one.view();
  std::vector<std::tuple<uint64_t, size_t, size_t>> pairs;
  for (size_t j = n0; j < n1; j++)
    for (size_t i = 0; i < j; i++) {
      uint64_t id = 0;
      if (index_group_pair(view, (uint32_t)i, (uint32_t)j, &id)) pairs.emplace_back(id, i, j);
    }
  std::sort(pairs.begin(), pairs.end());
  const uint64_t first = view.vbase[n0];
  std::vector<NeedleHipProblem> brute;
  uint64_t searched = 0;
  for (size_t q = 0; q < pairs.size(); q++) {
    const uint64_t id = std::get<0>(pairs[q]);
    const size_t i = std::get<1>(pairs[q]), j = std::get<2>(pairs[q]);
    CHECK(id == first + q, "%s %zu + %zu: the new ids are not [first, first + new)", what, n0, k);
    bool any = false;
    for (size_t r = 0; r < R; r++) {
      const uint32_t a = min_len[i * R + r], b = min_len[j * R + r];
      if (!a || !b) continue;
      brute.push_back(NeedleHipProblem{(uint32_t)(i * R + r), (uint32_t)(j * R + r), std::max(a, b), (uint32_t)((id - first) * R + r)});
      any = true;
    }
    searched += any;
  }
  CHECK(p.first_pair == first && p.new_pairs == pairs.size() && p.searched == searched && same(p.problems, brute), "%s %zu + %zu x %zu: brute force", what,
        n0, k, R);
  const IndexAppendPlan streamed = planned(n0, k, R, labels, min_len, IndexRoute::Streamed);
  const IndexAppendPlan scan = planned(n0, k, R, labels, min_len, IndexRoute::Scan);
  CHECK(same(streamed.problems, p.problems) && same(scan.problems, p.problems) && streamed.searched == p.searched && scan.searched == p.searched,
        "%s %zu + %zu: the route changes the list", what, n0, k);
  for (size_t r = 0; r < R; r++) {
    const uint32_t all = before::least(n0, n1, R, r, min_len, groups.get(), false), arriving = before::least(n0, n1, R, r, min_len, groups.get(), true);
    CHECK(p.least[r] == all && streamed.least[r] == arriving, "%s %zu + %zu region %zu: least %u / %u, brute force %u / %u", what, n0, k, r, p.least[r],
          streamed.least[r], all, arriving);
    g_saw_no_live_pair = g_saw_no_live_pair || (all == UINT32_MAX && n1 > 1);
  }
  check_ids(*p.ids, labels, n1, what);
}

// (3) the same plan with one label and with none
void check_one_label(size_t n0, size_t k, size_t R, const std::vector<uint32_t> &min_len) {
  const std::vector<uint32_t> labels(n0 + k, 7u);
  for (IndexRoute route : {IndexRoute::Scan, IndexRoute::Matched, IndexRoute::Streamed}) {
    const IndexAppendPlan a = planned(n0, k, R, nullptr, min_len, route), b = planned(n0, k, R, labels.data(), min_len, route);
    CHECK(a.n0 == b.n0 && a.n1 == b.n1 && a.regions == b.regions && a.first_pair == b.first_pair && a.new_pairs == b.new_pairs &&
              a.searched == b.searched && same(a.problems, b.problems) && a.least[0] == b.least[0] && a.least[1] == b.least[1],
          "one label %zu + %zu x %zu", n0, k, R);
    CHECK(!a.ids->labelled() && b.ids->labelled() && a.labels.empty() && b.labels == labels, "one label %zu + %zu: the flag", n0, k);
    CHECK(a.ids->pairs() == b.ids->pairs(), "one label %zu + %zu: pairs", n0, k);
    for (size_t v = 0; v <= n0 + k; v++) CHECK(a.ids->column(v) == b.ids->column(v), "one label %zu + %zu: column %zu", n0, k, v);
    for (size_t v = 0; v < n0 + k; v++) {
      CHECK(listed(a.ids->group(v)) == listed(b.ids->group(v)) && listed(a.ids->lower(v)) == listed(b.ids->lower(v)) &&
                a.ids->paired(v) == b.ids->paired(v),
            "one label %zu + %zu: partners of %zu", n0, k, v);
    }
  }
}

// (5) 0 -> n in one step against the steps `cuts` (ascending sizes of the list after each step, the last one n)
void check_composition(size_t R, const uint32_t *labels, size_t n, const std::vector<uint32_t> &min_len, const std::vector<size_t> &cuts) {
  typedef std::tuple<uint32_t, uint32_t, uint32_t, uint64_t> Listed;  // rows, min_len, absolute id x R + r
  auto listed = [&](const IndexAppendPlan &p, std::set<Listed> *into) {
    size_t fresh = 0;
    for (const NeedleHipProblem &pr : p.problems) fresh += into->insert(Listed(pr.src_seq, pr.dst_seq, pr.min_len, p.first_pair * R + pr.tag)).second;
    return fresh;
  };
  std::set<Listed> whole, parts;
  const IndexAppendPlan all = planned(0, n, R, labels, min_len, IndexRoute::Scan);
  CHECK(listed(all, &whole) == all.problems.size() && all.first_pair == 0, "composition: 0 -> %zu", n);
  size_t n0 = 0;
  uint64_t searched = 0;
  for (size_t n1 : cuts) {
    const std::vector<uint32_t> rows(min_len.begin(), min_len.begin() + n1 * R);
    const IndexAppendPlan step = planned(n0, n1 - n0, R, labels, rows, IndexRoute::Scan);
    CHECK(listed(step, &parts) == step.problems.size(), "composition: step %zu -> %zu of %zu lists a problem again", n0, n1, n);
    searched += step.searched;
    for (size_t j = 0; j < n1; j++)  // an append never renumbers a pair
      for (uint32_t i : step.ids->lower(j)) CHECK(step.ids->id(i, j) == all.ids->id(i, j), "composition: (%u, %zu) renumbered at %zu of %zu", i, j, n1, n);
    CHECK(step.ids->pairs() == all.ids->column(n1), "composition: %zu of %zu: pairs", n1, n);
    n0 = n1;
  }
  CHECK(n0 == n && whole == parts && searched == all.searched, "composition: %zu videos in %zu steps", n, cuts.size());
}

// (6) one edit: labels of the old list (null: none), n0 of them
void check_edit(const uint32_t *labels, size_t n0, const std::vector<uint32_t> &old_of_new, size_t R, std::mt19937 &rng, const char *what) {
  const size_t n1 = old_of_new.size();
  auto fresh = [&](size_t v) { return old_of_new[v] == kIndexPlanFresh; };
  const std::vector<uint32_t> old_labels(labels, labels + (labels ? n0 : 0));
  const IndexPairIds old_ids(labels, n0);
  const std::vector<uint32_t> one(n0, 0u);
  const IndexGroupTables old_tables(labels ? labels : one.data(), n0);  // the committed tables (a plain store has none: one label)
  const std::vector<uint32_t> min_len = some_min_len(rng, n1, R);
  IndexEditPlan p = plan_index_edit(old_ids, old_labels, old_of_new, R);
  CHECK(p.ids->too_large(R).ok(), "%s", what);
  list_index_edit(&p, old_of_new, min_len.data());
  std::vector<uint32_t> new_labels;
  for (size_t v = 0; v < n1 && labels; v++) new_labels.push_back(labels[fresh(v) ? v : old_of_new[v]]);
  CHECK(p.n0 == n0 && p.n1 == n1 && p.regions == R && p.labels == new_labels && p.ids->labelled() == (labels != nullptr), "%s: labels", what);
  check_ids(*p.ids, labels ? new_labels.data() : nullptr, n1, what);
  // against the loops index.cpp had
  std::unique_ptr<IndexGroupTables> groups(labels ? new IndexGroupTables(new_labels.data(), n1) : nullptr);
  const before::Edit want = before::edit(n0, old_of_new, R, min_len, groups.get());
  CHECK(p.new_of_old == want.new_of_old && p.gone == want.gone, "%s: new_of_old / gone", what);
  CHECK(p.pair_ids == want.pair_ids && same(p.problems, want.problems) && p.searched == want.searched, "%s: the listed pairs", what);
  // new_of_old and gone agree with old_of_new
  size_t kept = 0;
  for (size_t v = 0; v < n1; v++)
    if (!fresh(v)) kept += p.new_of_old[old_of_new[v]] == v;
  CHECK(kept + p.gone.size() == n0 && std::is_sorted(p.gone.begin(), p.gone.end()), "%s: kept %zu gone %zu of %zu", what, kept, p.gone.size(), n0);
  for (uint32_t q : p.gone) CHECK(q < n0 && p.new_of_old[q] == kIndexPlanFresh, "%s: gone %u", what, q);
  // brute force: every pair with a fresh end exactly once, under the later video where both are fresh, under its new id
  std::set<std::pair<size_t, size_t>> expected, got;
  for (size_t j = 0; j < n1; j++)
    for (size_t i = 0; i < j; i++)
      if ((fresh(i) || fresh(j)) && (!labels || new_labels[i] == new_labels[j])) expected.emplace(i, j);
  size_t owner = 0, tag = 0;
  for (size_t l = 0; l < p.pair_ids.size(); l++) {
    size_t i = 0, j = 0;
    CHECK(p.ids->at(p.pair_ids[l], &i, &j) && got.emplace(i, j).second, "%s: listed pair %zu", what, l);
    const size_t under = fresh(j) ? j : i;
    CHECK(under >= owner, "%s: listed pair %zu (%zu, %zu) is not under video %zu", what, l, i, j, under);
    owner = under;
    for (size_t r = 0; r < R; r++) {
      if (!min_len[i * R + r] || !min_len[j * R + r]) continue;
      CHECK(tag < p.problems.size() && p.problems[tag].tag == l * R + r && p.problems[tag].src_seq == i * R + r && p.problems[tag].dst_seq == j * R + r,
            "%s: problem %zu", what, tag);
      tag++;
    }
  }
  CHECK(got == expected && tag == p.problems.size(), "%s: %zu pairs listed, %zu have a fresh end", what, got.size(), expected.size());
  // a kept pair's old id through the old tables: what index_group_edit_buckets_kernel / index_edit_buckets_kernel map
  std::set<uint64_t> old_seen;
  for (uint64_t b = 0; b < p.ids->pairs(); b++) {
    size_t i = 0, j = 0;
    CHECK(p.ids->at(b, &i, &j), "%s: new id %llu", what, (unsigned long long)b);
    if (fresh(i) || fresh(j)) continue;
    const uint32_t oi = old_of_new[i], oj = old_of_new[j];
    uint64_t op = 0;
    size_t bi = 0, bj = 0;
    CHECK(oi < oj && index_group_pair(old_tables.view(), oi, oj, &op) && op == old_ids.id(oi, oj) && old_ids.at(op, &bi, &bj) && bi == oi && bj == oj &&
              old_seen.insert(op).second,
          "%s: the old id of kept pair (%zu, %zu)", what, i, j);
    if (!labels) CHECK(op == column_major_pair(oi, oj), "%s: the old id of kept pair (%zu, %zu), plain", what, i, j);
  }
  uint64_t kept_pairs = 0;  // old pairs with both ends kept
  for (size_t j = 0; j < n0; j++)
    for (uint32_t i : old_ids.lower(j)) kept_pairs += p.new_of_old[i] != kIndexPlanFresh && p.new_of_old[j] != kIndexPlanFresh;
  CHECK(old_seen.size() == kept_pairs, "%s: %zu kept pairs found, %llu exist", what, old_seen.size(), (unsigned long long)kept_pairs);
  // one label equals none
  if (!labels) {
    const std::vector<uint32_t> ones(n0, 3u);
    IndexEditPlan q = plan_index_edit(IndexPairIds(ones.data(), n0), ones, old_of_new, R);
    list_index_edit(&q, old_of_new, min_len.data());
    CHECK(q.new_of_old == p.new_of_old && q.gone == p.gone && q.pair_ids == p.pair_ids && same(q.problems, p.problems) && q.searched == p.searched &&
              q.ids->pairs() == p.ids->pairs() && q.ids->labelled() && q.labels == std::vector<uint32_t>(n1, 3u),
          "%s: one label", what);
  }
}

std::vector<uint32_t> removal(size_t n0, const std::vector<size_t> &positions) {
  std::vector<uint32_t> old_of_new;
  for (size_t q = 0; q < n0; q++)
    if (std::find(positions.begin(), positions.end(), q) == positions.end()) old_of_new.push_back((uint32_t)q);
  return old_of_new;
}
std::vector<uint32_t> replacement(size_t n0, const std::vector<size_t> &positions) {
  std::vector<uint32_t> old_of_new(n0);
  for (size_t q = 0; q < n0; q++) old_of_new[q] = std::find(positions.begin(), positions.end(), q) == positions.end() ? (uint32_t)q : kIndexPlanFresh;
  return old_of_new;
}

// ---- (8) acceptance ---------------------------------------------------------------------------------------------------------
struct Case {  // what a route's entry point is handed, accepted as it stands
  IndexAcceptance facts;
  std::vector<uint64_t> row_len;
  uint32_t least[2];
};

IndexRefusal first_refusal(const Case &c, const uint32_t **labels) {  // the stages in index.cpp's order
  IndexRefusal no = index_accept(c.facts, labels);
  if (no.ok()) no = index_accept_rows(c.facts, c.row_len.data());
  if (no.ok()) no = index_accept_min_len(c.facts, c.least);
  return no;
}

const uint32_t kIndexLabels[4] = {1, 2, 1, 2}, kMatcherLabels[6] = {1, 2, 1, 2, 2, 1};

Case accepted(IndexRoute route) {
  Case c;
  IndexAcceptance &f = c.facts;
  f.route = route;
  f.index_id = 7;
  f.generation = 3;
  f.device = 2;
  f.n0 = 4;
  f.k = 2;
  f.regions = 2;
  f.labels = route == IndexRoute::MatchedGrouped ? kIndexLabels : nullptr;
  c.row_len = {11, 12, 13, 0};
  c.least[0] = 5;
  c.least[1] = UINT32_MAX;
  auto fill = [&](IndexSource *s) {
    s->present = true;
    s->origin_id = 7;
    s->origin_generation = 3;
    s->device = 2;
    s->complete = true;
    s->lanes = 4;
    s->regions = 2;
    s->fed = c.row_len;
  };
  if (route == IndexRoute::Streamed) {
    fill(&f.matcher);
    fill(&f.cross);
    f.cross.origin_id = 0;  // made by needle_hip_crossmatcher_new_regions: of no index
    f.cross.origin_generation = 0;
    f.cross.min_len[0] = 5;
    f.cross.min_len[1] = 9;
  } else if (route != IndexRoute::Scan) {
    fill(&f.cross);
    f.cross.residents = 4;
    f.cross.min_len[0] = 5;
    f.cross.min_len[1] = 9;
    if (route == IndexRoute::MatchedGrouped) {
      f.cross.grouped = true;
      f.cross.labels = kMatcherLabels;
      f.cross.num_labels = 6;
    }
  }
  return c;
}

struct Stage {  // one place in the chain: the flips that raise its refusal
  NeedleError code;
  std::string text;
  std::vector<std::function<void(Case *)>> flips;
};

void check_chain(IndexRoute route, const char *what, const std::vector<Stage> &chain) {
  const uint32_t *const untouched = kIndexLabels + 1;
  const uint32_t *labels = untouched;
  const Case ok = accepted(route);
  const IndexRefusal none = first_refusal(ok, &labels);
  CHECK(none.ok() && none.text.empty(), "%s: the accepted facts are refused: %s", what, none.text.c_str());
  CHECK(labels == (route == IndexRoute::MatchedGrouped ? kMatcherLabels + 4 : untouched), "%s: the arriving videos' labels", what);
  for (size_t s = 0; s < chain.size(); s++)
    for (size_t a = 0; a < chain[s].flips.size(); a++) {
      Case one = ok;
      chain[s].flips[a](&one);
      labels = untouched;
      IndexRefusal no = first_refusal(one, &labels);
      CHECK(no.code == chain[s].code && no.text == chain[s].text, "%s: stage %zu flip %zu says \"%s\"", what, s, a, no.text.c_str());
      for (size_t b = 0; s + 1 < chain.size() && b < chain[s + 1].flips.size(); b++) {  // with the next stage's too: the earlier one wins
        Case two = one;
        chain[s + 1].flips[b](&two);
        no = first_refusal(two, &labels);
        CHECK(no.code == chain[s].code && no.text == chain[s].text, "%s: stage %zu flip %zu with stage %zu flip %zu says \"%s\"", what, s, a, s + 1, b,
              no.text.c_str());
      }
    }
}

void check_acceptance() {
  const NeedleError inv = NeedleError_InvalidArgument;
  const IndexRefusal poison{NeedleError_Unknown, "matcher: hipErrorUnknown in an earlier feed"};
  const IndexRefusal cross_poison{NeedleError_IOError, "crossmatcher: an earlier feed failed"};
  auto cross = [](std::function<void(IndexSource *)> f) { return [f](Case *c) { f(&c->facts.cross); }; };
  auto matcher = [](std::function<void(IndexSource *)> f) { return [f](Case *c) { f(&c->facts.matcher); }; };
  auto fed_more = [](IndexSource *s) { s->fed[2]++; };
  auto fed_less = [](IndexSource *s) { s->fed[0]--; };
  const std::string m = "index add_matched: ", t = "index add_streamed: ";
  // add_matched on a plain index
  const std::vector<Stage> matched = {
      {cross_poison.code, cross_poison.text, {cross([=](IndexSource *s) { s->poison = cross_poison; })}},
      {inv, m + "the matcher was not created from this index", {cross([](IndexSource *s) { s->origin_id = 8; })}},
      {inv, m + "the index has changed since the matcher was created", {cross([](IndexSource *s) { s->origin_generation = 2; })}},
      {inv, m + "the matcher is on another device than the index", {cross([](IndexSource *s) { s->device = 0; })}},
      {inv, m + "the matcher is not complete", {cross([](IndexSource *s) { s->complete = false; })}},
      {inv, m + "not the matcher's number of videos",
       {cross([](IndexSource *s) { s->lanes = 6; }), cross([](IndexSource *s) { s->regions = 1; }), cross([](IndexSource *s) { s->residents = 3; })}},
      {inv, m + "the matcher has groups", {cross([](IndexSource *s) { s->grouped = true; })}},
      {inv, m + "a video's row is not as long as what its lane was fed", {cross(fed_more), cross(fed_less)}},
      {inv, m + "the matcher's min_len exceeds the shortest run a pair can hold", {cross([](IndexSource *s) { s->min_len[0] = 6; })}},
  };
  check_chain(IndexRoute::Matched, "add_matched", matched);
  // add_matched_grouped
  static const uint32_t other_resident[6] = {1, 2, 2, 2, 2, 1};
  std::vector<Stage> grouped = matched;
  grouped[6] = {inv, m + "the matcher has no groups (needle_hip_index_crossmatcher_new_grouped makes one)", {cross([](IndexSource *s) { s->grouped = false; })}};
  grouped.insert(grouped.begin() + 7, Stage{inv, m + "the matcher's labels are not the index's",
                                            {cross([](IndexSource *s) { s->num_labels = 5; }), cross([](IndexSource *s) { s->labels = other_resident; })}});
  check_chain(IndexRoute::MatchedGrouped, "add_matched_grouped", grouped);
  // add_streamed: the matcher made from the index, the arriving pairs' cross-matcher
  const std::vector<Stage> streamed = {
      {poison.code, poison.text, {matcher([=](IndexSource *s) { s->poison = poison; })}},
      {cross_poison.code, cross_poison.text, {cross([=](IndexSource *s) { s->poison = cross_poison; })}},
      {inv, t + "the matcher was not created from this index", {matcher([](IndexSource *s) { s->origin_id = 8; })}},
      {inv, t + "the index has changed since the matcher was created", {matcher([](IndexSource *s) { s->origin_generation = 4; })}},
      {inv, t + "the cross-matcher has resident videos (the arriving pairs come from needle_hip_crossmatcher_new_regions)",
       {cross([](IndexSource *s) { s->residents = 1; })}},
      {inv, t + "the matcher is on another device than the index", {matcher([](IndexSource *s) { s->device = 0; }), cross([](IndexSource *s) { s->device = 1; })}},
      {inv, t + "the matcher is not complete", {matcher([](IndexSource *s) { s->complete = false; }), cross([](IndexSource *s) { s->complete = false; })}},
      {inv, t + "not the matcher's number of videos",
       {matcher([](IndexSource *s) { s->lanes = 2; }), matcher([](IndexSource *s) { s->regions = 1; }), cross([](IndexSource *s) { s->lanes = 6; }),
        cross([](IndexSource *s) { s->regions = 1; })}},
      {inv, t + "a video's row is not as long as what its lane was fed", {cross(fed_more), matcher(fed_less)}},
      {inv, t + "the matcher's min_len exceeds the shortest run a pair can hold", {cross([](IndexSource *s) { s->min_len[0] = 6; })}},
  };
  check_chain(IndexRoute::Streamed, "add_streamed", streamed);
  // one video: no cross-matcher, and nothing of it is read
  Case alone = accepted(IndexRoute::Streamed);
  alone.facts.cross = IndexSource();
  alone.facts.cross.poison = cross_poison;
  alone.facts.cross.min_len[0] = 100;
  alone.facts.k = 1;
  alone.facts.matcher.lanes = 2;
  const uint32_t *labels = nullptr;
  CHECK(first_refusal(alone, &labels).ok() && !labels, "add_streamed with one video");
  // the scan judges nothing
  Case scan = accepted(IndexRoute::Scan);
  scan.facts.cross.poison = cross_poison;
  CHECK(first_refusal(scan, &labels).ok() && !labels, "the scan route");
}

// (4) the unlabelled list where pairs x R crosses kIndexMaxBuckets
void check_boundary(size_t R) {
  size_t n = (size_t)std::sqrt(2.0 * (double)kIndexMaxBuckets / (double)R);
  while ((uint64_t)n * (n - 1) / 2 * R >= kIndexMaxBuckets) n--;
  while ((uint64_t)(n + 1) * n / 2 * R < kIndexMaxBuckets) n++;  // n: the last size below, n + 1: the first above
  CHECK((uint64_t)n * (n - 1) / 2 * R < kIndexMaxBuckets && (uint64_t)(n + 1) * n / 2 * R >= kIndexMaxBuckets, "boundary x %zu: %zu", R, n);
  const IndexAppendPlan below = plan_index_append(n - 1, 1, R, std::vector<uint32_t>(), nullptr);
  size_t i = 0, j = 0;
  CHECK(below.refusal.ok() && below.ids->too_large(R).ok() && below.first_pair == (uint64_t)(n - 1) * (n - 2) / 2 && below.new_pairs == n - 1 &&
            below.ids->pairs() == (uint64_t)n * (n - 1) / 2 && below.ids->at(below.ids->pairs() - 1, &i, &j) && i == n - 2 && j == n - 1,
        "boundary x %zu: %zu videos", R, n);
  IndexAppendPlan above = plan_index_append(n, 1, R, std::vector<uint32_t>(), nullptr);
  const std::vector<uint32_t> min_len((n + 1) * R, 1u);
  const IndexRefusal no = list_index_append(&above, min_len.data(), IndexRoute::Scan);
  CHECK(above.refusal.ok() && no.code == NeedleError_InvalidArgument && no.text == "index too large: more than 2^32 hashes or sequence pairs" &&
            above.problems.empty() && above.problems.capacity() == 0 && above.searched == 0,
        "boundary x %zu: %zu videos: %s", R, n + 1, no.text.c_str());
  CHECK(above.ids->too_large(R).text == no.text, "boundary x %zu", R);
}

}  // namespace

int main() {
  std::mt19937 rng(20260117u);
  // 1, 3, 7: no labels
  for (size_t R = 1; R <= 2; R++)
    for (size_t n0 = 0; n0 < 40; n0++)
      for (size_t k = 1; n0 + k <= 40; k++) {
        const std::vector<uint32_t> min_len = some_min_len(rng, n0 + k, R, (n0 + k) % 5 == 0);
        check_append(n0, k, R, nullptr, min_len, "plain");
        if ((n0 + k) % 3 == 0 || k == 1) check_one_label(n0, k, R, min_len);
      }
  // 2, 4, 7: labels
  for (size_t R = 1; R <= 2; R++)
    for (size_t n = 1; n <= 40; n++)
      for (size_t L = 1; L <= 6; L++)
        for (int pattern = 0; pattern < 3; pattern++) {
          std::vector<uint32_t> labels(n);
          for (size_t v = 0; v < n; v++) labels[v] = 5 + 3 * (uint32_t)(pattern == 0 ? v % L : rng() % L);  // interleaved
          if (pattern == 2) {
            labels[n - 1] = 1000;             // a label of one member, which first appears among the arriving videos ...
            if (n >= 3) labels[0] = 999;      // ... and one among the old ones
            if (n >= 6) labels[n - 2] = labels[n - 3] = 998;  // one that arrives with two members
          }
          const std::vector<uint32_t> min_len = some_min_len(rng, n, R, n % 7 == 0);
          for (size_t n0 : std::set<size_t>{0, 1 % n, n / 3, n / 2, n >= 2 ? n - 2 : 0, n - 1}) check_append(n0, n - n0, R, labels.data(), min_len, "labelled");
          // 5
          std::vector<size_t> singles, random_cuts;
          for (size_t c = 1; c <= n; c++) {
            singles.push_back(c);
            if (c == n || rng() % 3 == 0) random_cuts.push_back(c);
          }
          if (n % 4 == 0 || n < 6) {
            check_composition(R, labels.data(), n, min_len, singles);
            check_composition(R, labels.data(), n, min_len, random_cuts);
            check_composition(R, nullptr, n, min_len, random_cuts);
            check_composition(R, labels.data(), n, min_len, {(n + 1) / 2, n});
          }
        }
  CHECK(g_saw_no_live_pair, "no case had a region without a live pair");
  for (size_t R = 1; R <= 2; R++) check_boundary(R);
  const IndexAppendPlan crowd = plan_index_append((size_t)kIndexMaxVideos - 1, 1, 1, std::vector<uint32_t>(), nullptr);
  CHECK(crowd.refusal.code == NeedleError_InvalidArgument && crowd.refusal.text == "index too large: more than 2^32 videos" && !crowd.ids, "2^32 videos");
  // 6: nine videos, groups {0, 2, 6, 8} {1, 4} {3} {5, 7}
  const uint32_t shows[9] = {10, 20, 10, 30, 20, 40, 10, 40, 10};
  struct Named {
    const char *what;
    std::vector<uint32_t> old_of_new;
  };
  const std::vector<Named> edits = {
      {"remove the first", removal(9, {0})},          {"remove one in the middle", removal(9, {4})},
      {"remove the last", removal(9, {8})},           {"remove several", removal(9, {1, 4, 5})},
      {"remove a group of one", removal(9, {3})},     {"remove a whole group", removal(9, {5, 7})},
      {"remove all but one", removal(9, {0, 1, 2, 3, 4, 5, 6, 7})},
      {"replace the first", replacement(9, {0})},     {"replace the last", replacement(9, {8})},
      {"replace two neighbours", replacement(9, {3, 4})}, {"replace two of one group", replacement(9, {2, 6})},
      {"replace a group of one", replacement(9, {3})}, {"replace every video", replacement(9, {0, 1, 2, 3, 4, 5, 6, 7, 8})},
  };
  for (size_t R = 1; R <= 2; R++)
    for (const Named &e : edits) {
      check_edit(shows, 9, e.old_of_new, R, rng, (std::string(e.what) + ", labelled").c_str());
      check_edit(nullptr, 9, e.old_of_new, R, rng, (std::string(e.what) + ", plain").c_str());
    }
  for (int rep = 0; rep < 300; rep++) {  // and at random
    const size_t n0 = 1 + rng() % 24, R = 1 + rng() % 2, L = 1 + rng() % 6;
    std::vector<uint32_t> labels(n0);
    for (uint32_t &l : labels) l = rng() % L;
    std::vector<size_t> positions;
    for (size_t q = 0; q < n0; q++)
      if (rng() % 4 == 0) positions.push_back(q);
    if (positions.size() == n0) positions.pop_back();
    const std::vector<uint32_t> old_of_new = rep % 2 ? removal(n0, positions) : replacement(n0, positions);
    check_edit(rep % 3 ? labels.data() : nullptr, n0, old_of_new, R, rng, rep % 2 ? "a random removal" : "a random replacement");
  }
  check_acceptance();
  if (g_failed) {
    std::printf("%d invariants broken\n", g_failed);
    return 1;
  }
  std::printf("index plan ok\n");
  return 0;
}
