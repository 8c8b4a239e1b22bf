// The host plan of the incremental index (index.cpp executes it): which pairs an append or an edit lists, under which ids and
// tags, what it refuses on counts alone, and whether the objects that come with a streamed route are accepted -- in plain C++,
// no HIP types, no comparator, no store, so that it can be checked without a device (tests/cpp/index_plan_check.cpp).
//
// One numbering: the append-stable grouped id of pair_ids.h (IndexGroupView), id(i, j) = vbase[j] + rank_of[i].  A list
// without labels is planned as ONE label: the rank is the position, vbase[j] = j (j - 1) / 2 and the id is
// column_major_pair(i, j), the plain store's.  IndexPairIds answers for both, and is the only place that tells them apart.
// That holds on the host only: store_groups() is null for a plain list, which is how the store selects its closed-form
// kernels (index_store.h).
//
// What stays in index.cpp: the row tables (fresh_row, the kept rows' gather, timestamp sharing), which need the comparator and
// the videos' data, the test for ending data (it asks paired() here), the store calls and the commit.  Their refusals fall
// between the plan's, so the plan is asked in stages: index_accept, plan_index_append, index_accept_rows, list_index_append,
// index_accept_min_len for an append; plan_index_edit, IndexPairIds::too_large, list_index_edit for an edit.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/needle_hip.h"
#include "pair_ids.h"

namespace needle {

constexpr uint32_t kIndexPlanFresh = 0xFFFFFFFFu;         // old_of_new[v] of a replacement (index_store.h: kIndexFresh)
constexpr uint64_t kIndexMaxBuckets = 0xFFFFFFF0ull;      // pairs x regions below this: problem tags and bucket ids are 32-bit on the device
constexpr uint64_t kIndexMaxVideos = 0xFFFFFFFFull;

struct IndexRefusal {  // what becomes the Status of the call
  NeedleError code = NeedleError_Ok;
  std::string text;
  bool ok() const { return code == NeedleError_Ok; }
};

// ---- a. the pair ids of one list ---------------------------------------------------------------------------------------
// Labelled: pair_ids.h's tables over the labels.  Not labelled: one label, whose tables would say rank = position and
// vbase[v] = v (v - 1) / 2 -- answered by that arithmetic, since the tables of a large plain list cost as much host time as
// the rest of a small append and the plain store wants none.
class IndexPairIds {
 public:
  struct Members {  // list positions, ascending: table[0 .. count), or 0 .. count - 1 themselves where there is no table
    const uint32_t *table;
    uint32_t count;
    struct Iterator {
      const uint32_t *table;
      uint32_t at;
      uint32_t operator*() const { return table ? table[at] : at; }
      Iterator &operator++() { return at++, *this; }
      bool operator!=(const Iterator &o) const { return at != o.at; }
    };
    Iterator begin() const { return Iterator{table, 0}; }
    Iterator end() const { return Iterator{table, count}; }
  };

  IndexPairIds(const uint32_t *labels, size_t n) : n_(n), tables_(labels ? new IndexGroupTables(labels, n) : nullptr) {}

  bool labelled() const { return tables_ != nullptr; }
  // IndexOptions::groups: null for a plain list
  const IndexGroupTables *store_groups() const { return tables_.get(); }
  size_t videos() const { return n_; }
  uint64_t pairs() const { return column(n_); }
  // the id at which video v's column starts; column(videos()) = pairs()
  uint64_t column(uint64_t v) const { return tables_ ? tables_->vbase[v] : v * (v - 1) / 2; }
  bool together(size_t i, size_t j) const { return !tables_ || tables_->group_of[i] == tables_->group_of[j]; }
  // i < j, the two together
  uint64_t id(size_t i, size_t j) const { return column(j) + (tables_ ? tables_->rank_of[i] : i); }
  // exact, by bisection: the last video whose column starts at or before `id`
  bool at(uint64_t id, size_t *i, size_t *j) const {
    uint32_t a = 0, b = 0;
    if (tables_) {
      if (!index_group_pair_at(tables_->view(), id, &a, &b)) return false;
    } else {
      if (id >= pairs()) return false;
      uint64_t lo = 1, hi = n_ - 1;
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (column(mid) <= id) lo = mid;
        else hi = mid - 1;
      }
      a = (uint32_t)(id - column(lo));
      b = (uint32_t)lo;
    }
    *i = a;
    *j = b;
    return true;
  }
  // j's lower partners: the q-th of them, i, has id(i, j) = column(j) + q
  Members lower(size_t j) const { return Members{group(j).table, (uint32_t)(tables_ ? tables_->rank_of[j] : j)}; }
  // v and all its partners
  Members group(size_t v) const {
    if (!tables_) return Members{nullptr, (uint32_t)n_};
    const uint32_t g = tables_->group_of[v];
    return Members{tables_->members.data() + tables_->first[g], tables_->size[g]};
  }
  bool paired(size_t v) const { return group(v).count > 1; }  // is v in any pair
  // the refusal on the pair count alone, before anything proportional to it is allocated or enumerated
  IndexRefusal too_large(size_t regions) const {
    if (pairs() * regions < kIndexMaxBuckets) return IndexRefusal();
    return IndexRefusal{NeedleError_InvalidArgument, "index too large: more than 2^32 hashes or sequence pairs"};
  }

 private:
  size_t n_;
  std::unique_ptr<const IndexGroupTables> tables_;
};

// ---- c. acceptance of a streamed source ------------------------------------------------------------------------------------
// Scan: add / add_grouped.  Matched, MatchedGrouped: a cross-matcher made from the index (add_matched on a plain index,
// add_matched_grouped on a grouped one).  Streamed: a matcher made from the index and, for more than one video, a cross-matcher
// over the arriving videos alone (add_streamed).
enum class IndexRoute { Scan, Matched, MatchedGrouped, Streamed };

struct IndexSource {  // what a Matcher or a CrossMatcher says of itself
  bool present = false;
  IndexRefusal poison;                            // its standing error, passed on as it is; nothing else is filled then
  uint64_t origin_id = 0, origin_generation = 0;  // the index it was made from, and that index's generation then
  int device = 0;
  bool complete = false;  // every lane finished
  size_t lanes = 0;       // videos x regions
  size_t regions = 0, residents = 0;
  bool grouped = false;
  const uint32_t *labels = nullptr;  // a grouped cross-matcher's, residents first
  size_t num_labels = 0;
  std::vector<uint64_t> fed;      // items fed, per lane
  uint32_t min_len[2] = {0, 0};   // per region (a cross-matcher's)
};

struct IndexAcceptance {
  IndexRoute route = IndexRoute::Scan;
  uint64_t index_id = 0, generation = 0;
  int device = 0;
  size_t n0 = 0, k = 0, regions = 1;
  const uint32_t *labels = nullptr;  // the index's n0 labels (a grouped index)
  IndexSource matcher;               // Streamed
  IndexSource cross;                 // Matched, MatchedGrouped; Streamed: the arriving pairs' (absent with one video)
};

inline IndexRefusal index_route_refusal(IndexRoute route, const char *what) {
  return IndexRefusal{NeedleError_InvalidArgument, std::string(route == IndexRoute::Streamed ? "index add_streamed: " : "index add_matched: ") + what};
}

// The first stage: everything known before a row is looked at.  *arriving_labels: MatchedGrouped sets it to the matcher's.
inline IndexRefusal index_accept(const IndexAcceptance &f, const uint32_t **arriving_labels) {
  auto refuse = [&](const char *what) { return index_route_refusal(f.route, what); };
  const IndexSource &mt = f.matcher, &cm = f.cross;
  const size_t k = f.k, R = f.regions;
  if (f.route == IndexRoute::Streamed) {
    if (!mt.poison.ok()) return mt.poison;
    if (cm.present && !cm.poison.ok()) return cm.poison;
    if (mt.origin_id != f.index_id) return refuse("the matcher was not created from this index");
    if (mt.origin_generation != f.generation) return refuse("the index has changed since the matcher was created");
    if (cm.present && cm.residents != 0)
      return refuse("the cross-matcher has resident videos (the arriving pairs come from needle_hip_crossmatcher_new_regions)");
    if (mt.device != f.device || (cm.present && cm.device != f.device)) return refuse("the matcher is on another device than the index");
    if (!mt.complete || (cm.present && !cm.complete)) return refuse("the matcher is not complete");
    if (k * R != mt.lanes || R != mt.regions || (cm.present && (k * R != cm.lanes || R != cm.regions)))
      return refuse("not the matcher's number of videos");
  } else if (f.route != IndexRoute::Scan) {
    const bool grouped = f.route == IndexRoute::MatchedGrouped;
    if (!cm.poison.ok()) return cm.poison;
    if (cm.origin_id != f.index_id) return refuse("the matcher was not created from this index");
    if (cm.origin_generation != f.generation) return refuse("the index has changed since the matcher was created");
    if (cm.device != f.device) return refuse("the matcher is on another device than the index");
    if (!cm.complete) return refuse("the matcher is not complete");
    if (k * R != cm.lanes || R != cm.regions || f.n0 != cm.residents) return refuse("not the matcher's number of videos");
    if (grouped != cm.grouped)
      return refuse(grouped ? "the matcher has no groups (needle_hip_index_crossmatcher_new_grouped makes one)" : "the matcher has groups");
    if (grouped) {  // the arriving videos' labels are the matcher's
      if (cm.num_labels != f.n0 + k || !std::equal(f.labels, f.labels + f.n0, cm.labels)) return refuse("the matcher's labels are not the index's");
      *arriving_labels = cm.labels + f.n0;
    }
  }
  return IndexRefusal();
}

// The second stage: row_len[lane] of the k x regions arriving rows against what each object's lane was fed.
inline IndexRefusal index_accept_rows(const IndexAcceptance &f, const uint64_t *row_len) {
  for (const IndexSource *from : {&f.cross, &f.matcher})
    for (size_t lane = 0; from->present && lane < f.k * f.regions; lane++)
      if (row_len[lane] != from->fed[lane]) return index_route_refusal(f.route, "a video's row is not as long as what its lane was fed");
  return IndexRefusal();
}

// The third: the cross-matcher had one min_len per region, a lower bound: beyond the smallest bound of a live pair it covered
// (IndexAppendPlan::least) it has lost runs.
inline IndexRefusal index_accept_min_len(const IndexAcceptance &f, const uint32_t *least) {
  for (size_t r = 0; f.cross.present && r < f.regions; r++)
    if (f.cross.min_len[r] > least[r]) return index_route_refusal(f.route, "the matcher's min_len exceeds the shortest run a pair can hold");
  return IndexRefusal();
}

// ---- b. the plan of an append and of an edit -------------------------------------------------------------------------------
// The problems of pair (i, j), tagged from `tag` on; min_len and the regions left out as in run_with_frame_hashes (one of
// whose sequences can hold no run long enough).  Whether any region is searched.  least[r] (where given): the smallest
// max(min_len) of a live pair so far.
inline bool index_pair_problems(const uint32_t *min_len, size_t R, size_t i, size_t j, uint64_t tag, std::vector<NeedleHipProblem> *problems,
                                uint32_t *least = nullptr) {
  bool any = false;
  for (size_t r = 0; r < R; r++) {
    const uint32_t a = min_len[i * R + r], b = min_len[j * R + r];
    if (a == 0 || b == 0) continue;
    problems->push_back(NeedleHipProblem{(uint32_t)(i * R + r), (uint32_t)(j * R + r), std::max(a, b), (uint32_t)(tag + r)});
    if (least) least[r] = std::min(least[r], std::max(a, b));
    any = true;
  }
  return any;
}

// Videos [n0, n0 + k) join n0.  The new pairs are each arriving video's with its lower partners, old and arriving alike, in
// ascending id: [first_pair, first_pair + new_pairs), since an append adds ids only at the end.
struct IndexAppendPlan {
  IndexRefusal refusal;  // of plan_index_append; nothing else holds then
  size_t n0 = 0, n1 = 0, regions = 1;
  std::vector<uint32_t> labels;             // of all n1 videos; empty without labels
  std::unique_ptr<const IndexPairIds> ids;  // of the list after the append
  uint64_t first_pair = 0, new_pairs = 0;
  // list_index_append:
  std::vector<NeedleHipProblem> problems;   // tag = (id - first_pair) * regions + region
  uint64_t searched = 0;                    // new pairs with a problem
  uint32_t least[2] = {UINT32_MAX, UINT32_MAX};  // per region, over the live pairs a matcher covered: all of them, on the
                                                 // streamed route the arriving x arriving ones (UINT32_MAX: none)
};

// new_labels null: a list without labels (old_labels is not read).
inline IndexAppendPlan plan_index_append(size_t n0, size_t k, size_t R, const std::vector<uint32_t> &old_labels, const uint32_t *new_labels) {
  IndexAppendPlan p;
  p.n0 = n0;
  p.n1 = n0 + k;
  p.regions = R;
  if (p.n1 >= kIndexMaxVideos) {
    p.refusal = IndexRefusal{NeedleError_InvalidArgument, "index too large: more than 2^32 videos"};
    return p;
  }
  if (new_labels) {
    p.labels = old_labels;
    p.labels.insert(p.labels.end(), new_labels, new_labels + k);
  }
  p.ids.reset(new IndexPairIds(new_labels ? p.labels.data() : nullptr, p.n1));
  p.first_pair = p.ids->column(n0);
  p.new_pairs = p.ids->pairs() - p.first_pair;
  return p;
}

// min_len: of all n1 x regions rows after the append.  The refusal on counts comes before anything is enumerated.
inline IndexRefusal list_index_append(IndexAppendPlan *p, const uint32_t *min_len, IndexRoute route) {
  const IndexPairIds &ids = *p->ids;
  const size_t R = p->regions;
  const IndexRefusal no = ids.too_large(R);
  if (!no.ok()) return no;
  p->problems.reserve(p->new_pairs * R);
  for (size_t j = p->n0; j < p->n1; j++) {
    uint64_t id = ids.column(j);
    for (uint32_t i : ids.lower(j)) {
      const bool covered = route != IndexRoute::Streamed || i >= p->n0;
      p->searched += index_pair_problems(min_len, R, i, j, (id++ - p->first_pair) * R, &p->problems, covered ? p->least : nullptr);
    }
  }
  return IndexRefusal();
}

// The list becomes old_of_new[v] (an old position) or, where that is kIndexPlanFresh, a fresh video in place of position v.
// A kept video keeps its label, a replacement the label of the position it replaces; groups are numbered and ranked again
// over the new list (a group that is emptied renumbers the later ones, a removed member lowers the ranks behind it).
struct IndexEditPlan {
  size_t n0 = 0, n1 = 0, regions = 1;
  std::vector<uint32_t> new_of_old;  // [n0]: the new position of a video kept, or kIndexPlanFresh (removed or replaced)
  std::vector<uint32_t> gone;        // the old positions removed or replaced, ascending
  std::vector<uint32_t> labels;      // of the new list; empty without labels
  std::unique_ptr<const IndexPairIds> ids;  // of the new list
  // list_index_edit: the pairs with a fresh video, each once (two fresh videos: under the later one)
  std::vector<uint32_t> pair_ids;          // listed pair -> its id under `ids`
  std::vector<NeedleHipProblem> problems;  // tag = listed pair * regions + region
  uint64_t searched = 0;
};

// committed: the ids of the list as it is; its labels are read where it has any.
inline IndexEditPlan plan_index_edit(const IndexPairIds &committed, const std::vector<uint32_t> &old_labels, const std::vector<uint32_t> &old_of_new,
                                     size_t R) {
  const bool labelled = committed.labelled();
  const size_t n0 = committed.videos();
  IndexEditPlan p;
  p.n0 = n0;
  p.n1 = old_of_new.size();
  p.regions = R;
  p.new_of_old.assign(n0, kIndexPlanFresh);
  for (size_t v = 0; v < p.n1; v++) {
    const bool fresh = old_of_new[v] == kIndexPlanFresh;
    if (!fresh) p.new_of_old[old_of_new[v]] = (uint32_t)v;
    if (labelled) p.labels.push_back(old_labels[fresh ? v : old_of_new[v]]);
  }
  for (size_t q = 0; q < n0; q++)
    if (p.new_of_old[q] == kIndexPlanFresh) p.gone.push_back((uint32_t)q);
  p.ids.reset(new IndexPairIds(labelled ? p.labels.data() : nullptr, p.n1));
  return p;
}

// min_len: of all n1 x regions rows of the new list.  After p->ids->too_large(regions) had nothing to say: that refusal comes
// before the new list's rows are made.
inline void list_index_edit(IndexEditPlan *p, const std::vector<uint32_t> &old_of_new, const uint32_t *min_len) {
  const IndexPairIds &ids = *p->ids;
  auto fresh = [&](size_t v) { return old_of_new[v] == kIndexPlanFresh; };
  auto list = [&](size_t i, size_t j) {
    p->searched += index_pair_problems(min_len, p->regions, i, j, (uint64_t)p->pair_ids.size() * p->regions, &p->problems);
    p->pair_ids.push_back((uint32_t)ids.id(i, j));
  };
  for (size_t f = 0; f < p->n1; f++) {
    if (!fresh(f)) continue;
    for (uint32_t q : ids.group(f)) {
      if (q < f) list(q, f);
      else if (q > f && !fresh(q)) list(f, q);
    }
  }
}

}  // namespace needle
