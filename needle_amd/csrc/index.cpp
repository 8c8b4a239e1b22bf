// NeedleHipIndex: an incremental search index (include/needle_hip.h, "Incremental index"; DESIGN.md "Incremental index").
//
// find_best_match for video v (comparator.rs:405-515) is a pure function of v's candidate list: its pairs' heap entries in
// the reference's pair order, (q, v) for q < v, then (v, q) for q > v (:414-431, 534-545).  When videos are only APPENDED,
// every existing pair keeps its source / destination roles, and every new pair of an old video v is (v, new), after all
// of v's old pairs in the full search over the concatenated list.  So keeping every pair's entries, computing entries for
// the new pairs only and re-running best_match for the videos whose candidate list changed is bit-identical to
// Comparator::run_with_frame_hashes over all videos in insertion order.  The entries live on the device (index_store.hip,
// IndexStore) under column-major pair ids p(i, j) = j (j - 1) / 2 + i, which do not depend on the number of videos.
//
// A GROUPED index holds a label per video and only the pairs inside a group: the same argument per group, since
// restricting a candidate list to a group keeps the relative order of what is left.  Its ids are pair_ids.h's IndexGroupView
// ids, the column-major id generalised so that an append still adds ids only at the end, whichever group grows.
//
// What an operation lists, under which ids and tags, what it refuses on counts alone and whether a streamed route's objects
// are accepted is decided in index_plan.h, where a plain index is one label; this file makes the row tables,
// calls the store and commits.
#include "index.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <unordered_map>

#include "epilogue.h"
#include "index_store.h"

namespace needle {

namespace {

static_assert(kIndexPlanFresh == kIndexFresh, "the plan and the store mark a replacement alike");

Status refused(const IndexRefusal &r) { return Status::Make(r.code, r.text); }
IndexRefusal standing(const Status &s) { return IndexRefusal{s.code, s.message}; }

// A bucket the device does not order (beyond kEpilogueLargeLimit runs, or rows the packed keys cannot stand for): the entries
// of an operation's `buckets` buckets (tag = listed pair * R + region) from its run list, with the host form's own functions.
// id_of(listed pair) gives its id under `ids`.  start[b] is relative to the operation's first entry.
template <class IdOf, class RowSeq, class Video>
void host_entries(const Comparator &cmp, size_t R, uint64_t buckets, const std::vector<NeedleHipRun> &runs, const IndexPairIds &ids, IdOf id_of,
                  RowSeq row_seq, Video video, std::vector<uint32_t> *start_out, std::vector<uint32_t> *valid_out,
                  std::vector<IndexEntry> *entries_out) {
  std::vector<uint32_t> start(buckets + 1, 0), valid(buckets, 0);
  for (const NeedleHipRun &r : runs)
    if (r.problem < buckets) start[r.problem + 1]++;
  for (uint64_t b = 0; b < buckets; b++) start[b + 1] += start[b];
  std::vector<NeedleHipRun> sorted(start[buckets]);
  {
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (const NeedleHipRun &r : runs)
      if (r.problem < buckets) sorted[fill[r.problem]++] = r;
  }
  std::vector<IndexEntry> entries(runs.size());
  std::vector<HeapEntry> tmp;
  for (uint64_t b = 0; b < buckets; b++) {
    const uint32_t lo = start[b], hi = start[b + 1];
    if (hi == lo) continue;
    std::sort(sorted.begin() + lo, sorted.begin() + hi, [](const NeedleHipRun &x, const NeedleHipRun &y) {
      return x.src_end != y.src_end ? x.src_end > y.src_end : x.dst_end > y.dst_end;  // the reference's walk (:191-192)
    });
    const size_t r = b % R;
    size_t i = 0, j = 0;
    (void)ids.at(id_of(b / R), &i, &j);
    cmp.entries_from_runs(&sorted[lo], hi - lo, row_seq(i, r), row_seq(j, r), video(i).hash_duration, video(j).hash_duration, r == 0, &tmp);
    for (size_t q = 0; q < tmp.size(); q++) {
      const HeapEntry &e = tmp[q];
      entries[lo + q] = IndexEntry{e.src_start, e.src_end, e.dst_start, e.dst_end, (uint32_t)e.score, e.src_match_hash, e.dst_match_hash, 0u};
    }
    valid[b] = (uint32_t)tmp.size();
  }
  start.pop_back();
  start_out->swap(start);
  valid_out->swap(valid);
  entries_out->swap(entries);
}

// After gpu_index_append / gpu_index_edit.  A bucket the device does not order: the operation's entries are computed here from
// its run list and given back through upload(start, valid, entries), which runs its second half again.  Then the failure count.
template <class IdOf, class RowSeq, class Video, class Upload>
Status settle(const Comparator &cmp, const char *where, size_t R, uint64_t buckets, const IndexPairIds &ids, IdOf id_of, RowSeq row_seq,
              Video video, Upload upload, const IndexAppendOut &out) {
  if (out.failed & kEpilogueBucketTooLarge) {
    note_epilogue_host_fallback(where, out.runs.size(), ids.videos());
    std::vector<uint32_t> start, valid;
    std::vector<IndexEntry> entries;
    host_entries(cmp, R, buckets, out.runs, ids, id_of, row_seq, video, &start, &valid, &entries);
    Status s = upload(start, valid, entries);  // (writes `out`)
    if (!s.ok()) return s;
  }
  if (out.failed)  // best_match_kernel: the winner's end minus padding / hash duration underflows (the reference panics)
    return Status::Make(NeedleError_Unknown, "overflow when subtracting durations (time_padding / hash_duration exceed the match end)");
  return Status::Ok();
}

// `ids`: of the list after the operation (evidence: the committed one's).  A plain list's store_groups() is null.
void set_options(const Comparator &cmp, size_t R, bool large_ok, const IndexPairIds &ids, IndexOptions *o) {
  o->groups = ids.store_groups();
  o->regions = (uint32_t)R;
  o->threshold = cmp.hash_match_threshold();
  o->include_endings = cmp.include_endings();
  o->large_ok = large_ok;
  o->min_opening_duration = cmp.min_opening_duration();
  o->min_ending_duration = cmp.min_ending_duration();
  o->time_padding = cmp.time_padding();
}

// Row `at` joins the index: its hashes (`hashes`) go behind the arena's, its timestamps (`ts`) behind the table's -- or, where
// they equal those of video 0's row of the same region (`first`, row `at % R`; null for video 0 itself), it reads that table,
// as in run_with_frame_hashes' device epilogue.  row_ok: what pair_entries_large_kernel's packed keys stand on.
Status fresh_row(const Comparator &cmp, const std::vector<HashTs> &seq, const std::vector<HashTs> *first, size_t R, size_t at, IndexRows *rows,
                 std::vector<uint32_t> *hashes, std::vector<uint64_t> *ts) {
  if (rows->hashes + seq.size() > UINT32_MAX)  // offsets into the arena are 32-bit on the device (NeedleHipSeq.offset)
    return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 hashes or sequence pairs");
  rows->seqs[at] = NeedleHipSeq{(uint32_t)rows->hashes, (uint32_t)seq.size()};
  rows->hashes += seq.size();
  for (const HashTs &h : seq) hashes->push_back(h.hash);
  rows->min_len[at] = cmp.min_run_length_for(seq, at % R == 0);
  bool same = first && seq.size() == first->size();
  for (size_t q = 0; q < seq.size() && same; q++) same = seq[q].ts == (*first)[q].ts;
  if (same) {
    rows->row_ts[at] = rows->row_ts[at % R];
  } else {
    rows->row_ts[at] = (uint32_t)rows->ts;
    for (const HashTs &h : seq) ts->push_back(h.ts);
    rows->ts += seq.size();
    if (rows->ts > UINT32_MAX) return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 timestamps");
  }
  bool ok = seq.size() < 65536u;
  for (size_t q = 1; q < seq.size() && ok; q++) ok = seq[q].ts > seq[q - 1].ts;
  rows->row_ok[at] = ok;
  return Status::Ok();
}

// The append fed from the route's objects in place of the scan.  Streamed: one list, the matcher's lanes first, and each of
// its runs' lanes; the new rows beside the histories of both objects.
Status append_streamed(IndexStore *store, const IndexAppend &a, const IndexRows &rows, Matcher *matcher, CrossMatcher *cross, IndexAppendOut *out) {
  const size_t first = (size_t)a.n0 * a.regions;
  std::vector<NeedleHipRun> list;
  std::vector<uint32_t> run_lane;
  for (size_t lane = 0; lane < a.num_rows; lane++) {
    const std::vector<NeedleHipRun> &runs = matcher->run_list(lane);
    list.insert(list.end(), runs.begin(), runs.end());
    run_lane.insert(run_lane.end(), runs.size(), (uint32_t)lane);
  }
  const size_t from_matcher = list.size();
  if (cross) list.insert(list.end(), cross->run_list().begin(), cross->run_list().end());
  std::vector<IndexLaneRow> lanes;
  for (size_t at = first; at < rows.seqs.size(); at++) {
    if (!rows.seqs[at].len) continue;
    if (const uint32_t *history = matcher->history(at - first)) lanes.push_back(IndexLaneRow{rows.seqs[at].offset, history, rows.seqs[at].len});
    if (cross) lanes.push_back(IndexLaneRow{rows.seqs[at].offset, cross->history(at - first), rows.seqs[at].len});
  }
  IndexStreamed m;
  m.runs = list.data();
  m.num_matcher_runs = from_matcher;
  m.num_cross_runs = list.size() - from_matcher;
  m.run_lane = run_lane.data();
  m.min_len = rows.min_len.data();
  m.lanes = lanes.data();
  m.num_lanes = lanes.size();
  return gpu_index_append_streamed(store, a, m, out);
}

Status append_matched(IndexStore *store, const IndexAppend &a, const IndexRows &rows, CrossMatcher *cross, IndexAppendOut *out) {
  const size_t first = (size_t)a.n0 * a.regions;
  std::vector<IndexSegment> lanes;
  for (size_t at = first; at < rows.seqs.size(); at++)
    if (rows.seqs[at].len)
      lanes.push_back(IndexSegment{rows.seqs[at].offset, (uint64_t)(cross->history(at - first) - cross->history(0)), rows.seqs[at].len});
  IndexMatched m;
  m.runs = cross->run_list().data();
  m.num_runs = cross->run_list().size();
  m.min_len = rows.min_len.data();
  m.history = cross->history(0);
  m.lanes = lanes.data();
  m.num_lanes = lanes.size();
  return gpu_index_append_matched(store, a, m, out);
}

const char *route_name(IndexRoute route) {
  return route == IndexRoute::Streamed ? "Index::add_streamed" : route == IndexRoute::Scan ? "Index::add" : "Index::add_matched";
}

std::atomic<uint64_t> next_index_id{1};

}  // namespace

Index::Index(const Comparator &comparator, bool grouped)
    : cmp_(comparator),
      include_endings_(comparator.include_endings()),
      regions_(comparator.include_endings() ? 2u : 1u),
      grouped_(grouped),
      id_(next_index_id++) {}

void Index::changed(uint64_t searched, uint64_t scanned) {
  pairs_last_ = searched;
  pairs_total_ += searched;
  scanned_last_ = scanned;
  scanned_total_ += scanned;
  generation_++;
}

Index::~Index() { index_store_free(store_); }

Status Index::init() {
  store_ = index_store_new();
  return Status::Ok();
}

Status Index::add(const std::vector<const FrameHashesData *> &fh) {
  if (grouped_)
    return Status::Make(NeedleError_InvalidArgument, "index add: a grouped index takes a label per video (needle_hip_index_add_grouped)");
  return append(fh, nullptr);
}

Status Index::add_grouped(const std::vector<const FrameHashesData *> &fh, const uint32_t *labels) {
  if (!labels) return Status::Make(NeedleError_NullArgument, "index add_grouped: null argument");
  if (!grouped_)
    return Status::Make(NeedleError_InvalidArgument, "index add_grouped: not a grouped index (needle_hip_index_new_grouped makes one)");
  return append(fh, labels);
}

// The plain streamed routes on a grouped index: their objects' runs name pairs across groups.  (A grouped cross-matcher has
// entry points of its own, crossmatcher_grouped / add_matched_grouped: DESIGN.md 6h; groups in the matcher are out of scope.)
Status Index::refuse_grouped(const char *route) const {
  return Status::Make(NeedleError_InvalidArgument, std::string("index ") + route + ": a grouped index has no streamed routes (use needle_hip_index_add_grouped)");
}

Status Index::add_matched(CrossMatcher *matcher, const std::vector<const FrameHashesData *> &fh) {
  if (grouped_) return refuse_grouped("add_matched");
  if (!matcher) return Status::Make(NeedleError_NullArgument, "index add_matched: null argument");
  return append(fh, nullptr, IndexRoute::Matched, matcher);
}

// The grouped index's streamed route: a grouped cross-matcher made by crossmatcher_grouped, whose labels name
// the arriving videos' groups.
Status Index::add_matched_grouped(CrossMatcher *matcher, const std::vector<const FrameHashesData *> &fh) {
  if (!matcher) return Status::Make(NeedleError_NullArgument, "index add_matched_grouped: null argument");
  if (!grouped_)
    return Status::Make(NeedleError_InvalidArgument, "index add_matched_grouped: not a grouped index (needle_hip_index_add_matched takes a plain one)");
  return append(fh, nullptr, IndexRoute::MatchedGrouped, matcher);
}

Status Index::add_streamed(Matcher *matcher, CrossMatcher *crossmatcher, const std::vector<const FrameHashesData *> &fh) {
  if (grouped_) return refuse_grouped("add_streamed");
  if (!matcher) return Status::Make(NeedleError_NullArgument, "index add_streamed: null argument");
  if (!crossmatcher && fh.size() > 1)
    return Status::Make(NeedleError_InvalidArgument, "index add_streamed: more than one video needs the cross-matcher of the arriving pairs");
  return append(fh, nullptr, IndexRoute::Streamed, crossmatcher, matcher);
}

// The index's rows as a matcher's sources (matcher.hip, regions): gathered on the device from the store's arena; a row's own
// min_len is a lower bound for every pair the row is in, and a row that can hold no run (min_len 0) has no cells.
Status Index::matcher(size_t videos, std::unique_ptr<Matcher> *out) {
  if (grouped_) return refuse_grouped("matcher");
  if (!out) return Status::Make(NeedleError_NullArgument, "index matcher: null argument");
  if (videos_.empty())
    return Status::Make(NeedleError_InvalidArgument,
                        "index matcher: an empty index has nothing resident (needle_hip_index_crossmatcher_new takes a first season)");
  if (videos == 0 || videos > 65535 / regions_) return Status::Make(NeedleError_InvalidArgument, "matcher: lanes must be 1 to 65535");
  // the argument checks first, with or without a device ...
  Status s = Matcher::CheckShape(rows_.hashes, rows_.seqs.data(), rows_.min_len.data(), rows_.seqs.size(), regions_, videos * regions_);
  if (!s.ok()) return s;
  // ... then the device, before anything is allocated on another one
  const uint32_t *d_hashes = nullptr;
  if (!(s = index_store_arena(store_, &d_hashes)).ok()) return s;
  std::unique_ptr<Matcher> mt;
  s = Matcher::CreateRegionsDevice(d_hashes, d_hashes ? rows_.hashes : 0, rows_.seqs.data(), rows_.min_len.data(), rows_.seqs.size(), regions_,
                                   videos * regions_, cmp_.hash_match_threshold(), &mt);
  if (!s.ok()) return s;
  mt->set_origin(Matcher::Origin{id_, generation_});
  *out = std::move(mt);
  return Status::Ok();
}

Status Index::crossmatcher(size_t videos, const size_t *max_items, const uint32_t *min_len, std::unique_ptr<CrossMatcher> *out) {
  if (grouped_) return refuse_grouped("crossmatcher");
  if (!out || !max_items || !min_len) return Status::Make(NeedleError_NullArgument, "crossmatcher: null argument");
  return make_crossmatcher(videos, nullptr, max_items, min_len, out);
}

// The grouped index's cross-matcher: the residents are the index's videos in index order under the index's labels, `groups` the
// arriving videos' labels; only the rows of the groups that arrive are gathered from the arena (crossmatch.hip).
Status Index::crossmatcher_grouped(size_t videos, const uint32_t *groups, const size_t *max_items, const uint32_t *min_len,
                                   std::unique_ptr<CrossMatcher> *out) {
  if (!out || !groups || !max_items || !min_len) return Status::Make(NeedleError_NullArgument, "crossmatcher: null argument");
  if (!grouped_)
    return Status::Make(NeedleError_InvalidArgument,
                        "index crossmatcher_grouped: not a grouped index (needle_hip_index_crossmatcher_new takes a plain one)");
  return make_crossmatcher(videos, groups, max_items, min_len, out);
}

Status Index::make_crossmatcher(size_t videos, const uint32_t *groups, const size_t *max_items, const uint32_t *min_len,
                                std::unique_ptr<CrossMatcher> *out) {
  CrossMatcher::Spec spec;
  spec.residents = videos_.size();
  spec.resident = rows_.seqs.data();
  spec.resident_groups = labels_.data();
  spec.arriving = videos;
  spec.groups = groups;
  spec.regions = regions_;
  spec.max_items = max_items;
  spec.min_len = min_len;
  spec.threshold = cmp_.hash_match_threshold();
  // The argument checks first, with or without a device (no state is asked for: the plan is host arithmetic) ...
  if (const char *what = CrossMatcher::ShapeError(spec)) return Status::Make(NeedleError_InvalidArgument, what);
  // ... then the device, before anything is allocated on another one
  const uint32_t *d_hashes = nullptr;
  Status s = index_store_arena(store_, &d_hashes);
  if (!s.ok()) return s;
  s = CrossMatcher::Create(spec, d_hashes, d_hashes ? rows_.hashes : 0, true, out);  // (which leaves *out alone where it fails)
  if (s.ok()) (*out)->set_origin(CrossMatcher::Origin{id_, generation_});
  return s;
}

// The facts index_accept() judges (index_plan.h).  A poisoned object says nothing but its standing error; otherwise no call
// below can fail: every lane asked for is one of the object's own.
IndexAcceptance Index::acceptance(IndexRoute route, size_t k, CrossMatcher *cross, Matcher *matcher) const {
  IndexAcceptance f;
  f.route = route;
  f.index_id = id_;
  f.generation = generation_;
  f.device = index_store_device(store_);
  f.n0 = videos_.size();
  f.k = k;
  f.regions = regions_;
  f.labels = labels_.data();
  if (matcher) {
    IndexSource &m = f.matcher;
    m.present = true;
    m.poison = standing(matcher->poisoned());
    if (m.poison.ok()) {
      m.origin_id = matcher->origin().index_id;
      m.origin_generation = matcher->origin().generation;
      m.device = matcher->device();
      m.lanes = matcher->lanes();
      m.regions = matcher->regions();
      m.fed.resize(m.lanes);
      m.complete = true;
      for (size_t lane = 0; lane < m.lanes; lane++) {
        bool finished = false;
        (void)matcher->Ready(lane, nullptr, &m.fed[lane], &finished);
        m.complete = m.complete && finished;
      }
    }
  }
  if (cross) {
    IndexSource &c = f.cross;
    c.present = true;
    c.poison = standing(cross->poisoned());
    if (c.poison.ok()) {
      c.origin_id = cross->origin().index_id;
      c.origin_generation = cross->origin().generation;
      c.device = cross->device();
      c.regions = cross->regions();
      c.lanes = cross->videos() * c.regions;
      c.residents = cross->residents();
      c.grouped = cross->grouped();
      c.labels = cross->labels().data();
      c.num_labels = cross->labels().size();
      (void)cross->Ready(nullptr, &c.complete);
      c.fed.resize(c.lanes);
      for (size_t lane = 0; lane < c.lanes; lane++) (void)cross->Lane(lane, &c.fed[lane], nullptr);
      for (size_t r = 0; r < c.regions && r < 2; r++) c.min_len[r] = cross->min_len(r);
    }
  }
  return f;
}

// Every add: facts -> plan -> rows -> IndexAppend -> the route's store call -> settle -> commit.  With a cross-matcher made from
// the index its runs stand in for the scan of the new pairs; with a matcher made from the index its runs stand in for the
// resident x arriving pairs and those of `cross`, a cross-matcher over the arriving videos alone (null: one video), for the
// arriving pairs.  `labels` (one per arriving video; MatchedGrouped: the cross-matcher's): a grouped index.
Status Index::append(const std::vector<const FrameHashesData *> &fh, const uint32_t *labels, IndexRoute route, CrossMatcher *cross,
                     Matcher *matcher) {
  if (fh.empty()) return Status::Make(NeedleError_InvalidArgument, "index add: no videos");
  const size_t k = fh.size(), n0 = videos_.size(), n1 = n0 + k, R = regions_;
  const IndexAcceptance from = acceptance(route, k, cross, matcher);
  IndexRefusal no = index_accept(from, &labels);
  if (!no.ok()) return refused(no);
  IndexAppendPlan plan = plan_index_append(n0, k, R, labels_, labels);
  if (!plan.refusal.ok()) return refused(plan.refusal);
  const IndexPairIds &ids = *plan.ids;
  auto video = [&](size_t v) -> const FrameHashesData & { return v < n0 ? videos_[v] : *fh[v - n0]; };
  auto row_seq = [&](size_t v, size_t r) -> const std::vector<HashTs> & { return r == 0 ? video(v).opening : video(v).ending; };
  if (include_endings_ && n1 > 1)
    for (size_t v = 0; v < n1; v++)
      if (video(v).ending.empty() && ids.paired(v))  // comparator.rs:271-273 (every video that is in some pair)
        return Status::Make(NeedleError_Unknown, "no ending hash data present");
  std::vector<uint64_t> arriving_len;
  for (size_t lane = 0; lane < k * R; lane++) arriving_len.push_back(row_seq(n0 + lane / R, lane % R).size());
  if (!(no = index_accept_rows(from, arriving_len.data())).ok()) return refused(no);
  IndexRows rows(rows_);
  rows.seqs.resize(n1 * R);
  rows.min_len.resize(n1 * R);
  rows.row_ts.resize(n1 * R);
  rows.row_ok.resize(n1 * R);
  std::vector<uint32_t> new_row_len, hashes;
  std::vector<uint64_t> ts, hash_duration;
  for (size_t v = n0; v < n1; v++) {
    hash_duration.push_back(video(v).hash_duration);
    for (size_t at = v * R; at < (v + 1) * R; at++) {
      Status s = fresh_row(cmp_, row_seq(v, at % R), v > 0 ? &row_seq(0, at % R) : nullptr, R, at, &rows, &hashes, &ts);
      if (!s.ok()) return s;
      new_row_len.push_back(rows.seqs[at].len);
      rows.large_ok = rows.large_ok && rows.row_ok[at];
    }
  }
  if (!(no = list_index_append(&plan, rows.min_len.data(), route)).ok()) return refused(no);
  if (!(no = index_accept_min_len(from, plan.least)).ok()) return refused(no);
  IndexAppend a;
  a.n0 = (uint32_t)n0;
  a.n1 = (uint32_t)n1;
  set_options(cmp_, R, rows.large_ok, ids, &a);
  a.hashes = hashes.data();
  a.num_hashes = hashes.size();
  a.seqs = rows.seqs.data();
  a.num_seqs = rows.seqs.size();
  a.problems = plan.problems.data();
  a.num_problems = plan.problems.size();
  a.row_len = new_row_len.data();
  a.row_ts = rows.row_ts.data() + n0 * R;
  a.num_rows = new_row_len.size();
  a.ts = ts.data();
  a.num_ts = ts.size();
  a.hash_duration = hash_duration.data();
  IndexAppendOut out;
  Status s = matcher ? append_streamed(store_, a, rows, matcher, cross, &out)
             : cross ? append_matched(store_, a, rows, cross, &out)
                     : gpu_index_append(store_, a, &out);
  if (!s.ok()) return s;
  if (out.refused & kIngestOtherHashes) return refused(index_route_refusal(route, "a video's hashes differ from what its lane was fed"));
  if (out.refused) return refused(index_route_refusal(route, "a run of the matcher does not lie inside its rows"));
  s = settle(cmp_, route_name(route), R, plan.new_pairs * R, ids, [&](uint64_t q) { return plan.first_pair + q; }, row_seq, video,
             [&](const auto &...computed) { return gpu_index_append_host_entries(store_, a, computed..., &out); }, out);
  if (!s.ok()) return s;
  // commit: nothing above changed the index
  index_store_commit(store_, a, out.found);
  for (const FrameHashesData *d : fh) videos_.push_back(*d);
  labels_.swap(plan.labels);
  ids_ = std::move(plan.ids);
  rows_ = std::move(rows);
  results_.resize(n1, NeedleHipSearchResult{});
  for (size_t q = 0; q < out.videos.size(); q++) results_[out.videos[q]] = out.results[q];
  changed(plan.searched, route == IndexRoute::Scan ? plan.searched : 0);
  return Status::Ok();
}

// Removal and replacement (DESIGN.md "Incremental index").  A pair's heap entries depend on the pair alone (its two sequences
// and which of them is the source: the one first in the list), and removal keeps the others' relative order, so every kept
// pair keeps its entries under its new id; a replacement keeps every position, and only the pairs of the replaced videos
// are searched again.  find_best_match is a function of a video's candidate list in pair order: it is recomputed for the
// fresh videos and for the videos with an entry in a pair that is dropped or new.  The store is rebuilt on the device.
Status Index::remove(const std::vector<size_t> &positions) {
  const size_t n0 = videos_.size();
  if (positions.empty()) return Status::Make(NeedleError_InvalidArgument, "index remove: no positions");
  std::vector<uint8_t> drop(n0, 0);
  for (size_t p : positions) {
    if (p >= n0) return Status::Make(NeedleError_InvalidArgument, "index remove: position out of range");
    if (drop[p]) return Status::Make(NeedleError_InvalidArgument, "index remove: repeated position");
    drop[p] = 1;
  }
  std::vector<uint32_t> old_of_new;
  for (size_t q = 0; q < n0; q++)
    if (!drop[q]) old_of_new.push_back((uint32_t)q);
  return rebuild(old_of_new, std::vector<const FrameHashesData *>(old_of_new.size(), nullptr));
}

Status Index::replace(const std::vector<size_t> &positions, const std::vector<const FrameHashesData *> &fh) {
  const size_t n0 = videos_.size();
  if (positions.empty() || positions.size() != fh.size()) return Status::Make(NeedleError_InvalidArgument, "index replace: no positions");
  std::vector<uint32_t> old_of_new(n0);
  std::vector<const FrameHashesData *> fresh(n0, nullptr);
  for (size_t q = 0; q < n0; q++) old_of_new[q] = (uint32_t)q;
  for (size_t k = 0; k < positions.size(); k++) {
    const size_t p = positions[k];
    if (p >= n0) return Status::Make(NeedleError_InvalidArgument, "index replace: position out of range");
    if (fresh[p]) return Status::Make(NeedleError_InvalidArgument, "index replace: repeated position");
    old_of_new[p] = kIndexFresh;
    fresh[p] = fh[k];
  }
  return rebuild(old_of_new, fresh);
}

// remove and replace: plan -> rows -> IndexEdit -> the store call -> settle -> commit.  The committed ids give a kept pair's
// old id (on the device: index_store.hip).
Status Index::rebuild(const std::vector<uint32_t> &old_of_new, const std::vector<const FrameHashesData *> &fresh) {
  const size_t n0 = videos_.size(), n1 = old_of_new.size(), R = regions_;
  if (n1 == 0) {  // every video removed: nothing is left to search or to hold
    index_store_clear(store_);
    videos_.clear();
    labels_.clear();
    ids_.reset();
    rows_ = IndexRows();
    results_.clear();
    changed(0, 0);
    return Status::Ok();
  }
  auto is_fresh = [&](size_t v) { return old_of_new[v] == kIndexFresh; };
  auto video = [&](size_t v) -> const FrameHashesData & { return is_fresh(v) ? *fresh[v] : videos_[old_of_new[v]]; };
  auto row_seq = [&](size_t v, size_t r) -> const std::vector<HashTs> & { return r == 0 ? video(v).opening : video(v).ending; };
  IndexEditPlan plan = plan_index_edit(*ids_, labels_, old_of_new, R);
  const IndexPairIds &ids = *plan.ids;
  if (include_endings_ && n1 > 1)
    for (size_t v = 0; v < n1; v++)
      if (video(v).ending.empty() && ids.paired(v))  // comparator.rs:271-273 (every video that is in some pair)
        return Status::Make(NeedleError_Unknown, "no ending hash data present");
  IndexRefusal no = ids.too_large(R);  // (before a row is made, as ever)
  if (!no.ok()) return refused(no);
  // The new rows.  Kept rows first, gathered on the device: their hashes in order, and each distinct run of the timestamp
  // table they read once (rows that shared video 0's timestamps keep sharing them, whichever video is removed).  Then the
  // fresh rows behind them, sharing the new video 0's timestamps where equal, as an append does.
  IndexRows rows(n1 * R);
  std::vector<uint32_t> row_len(n1 * R), hashes;
  std::vector<uint64_t> ts, hash_duration(n1);
  std::vector<IndexSegment> hash_rows, ts_rows;
  std::unordered_map<uint32_t, uint32_t> ts_at;  // a committed timestamp offset -> its offset in the new table
  for (size_t v = 0; v < n1; v++) {
    hash_duration[v] = video(v).hash_duration;
    if (is_fresh(v)) continue;
    for (size_t r = 0; r < R; r++) {
      const size_t row = v * R + r, orow = old_of_new[v] * R + r;
      const uint32_t len = rows_.seqs[orow].len;
      rows.seqs[row] = NeedleHipSeq{(uint32_t)rows.hashes, len};
      if (len) hash_rows.push_back(IndexSegment{rows_.seqs[orow].offset, rows.hashes, len});
      rows.hashes += len;
      rows.min_len[row] = rows_.min_len[orow];
      rows.row_ok[row] = rows_.row_ok[orow];
      row_len[row] = len;
      if (len == 0) continue;  // (row_ts 0: never read)
      auto it = ts_at.find(rows_.row_ts[orow]);
      if (it != ts_at.end()) {
        rows.row_ts[row] = it->second;
      } else {
        ts_at.emplace(rows_.row_ts[orow], (uint32_t)rows.ts);
        ts_rows.push_back(IndexSegment{rows_.row_ts[orow], rows.ts, len});
        rows.row_ts[row] = (uint32_t)rows.ts;
        rows.ts += len;
      }
    }
  }
  for (size_t v = 0; v < n1; v++) {
    if (!is_fresh(v)) continue;
    for (size_t at = v * R; at < (v + 1) * R; at++) {
      Status s = fresh_row(cmp_, row_seq(v, at % R), v > 0 ? &row_seq(0, at % R) : nullptr, R, at, &rows, &hashes, &ts);
      if (!s.ok()) return s;
      row_len[at] = rows.seqs[at].len;
    }
  }
  for (uint8_t ok : rows.row_ok) rows.large_ok = rows.large_ok && ok;
  list_index_edit(&plan, old_of_new, rows.min_len.data());
  IndexEdit e;
  e.n_old = (uint32_t)n0;
  e.n_new = (uint32_t)n1;
  set_options(cmp_, R, rows.large_ok, ids, &e);
  e.old_of_new = old_of_new.data();
  e.new_of_old = plan.new_of_old.data();
  e.gone = plan.gone.data();
  e.num_gone = plan.gone.size();
  e.hash_rows = hash_rows.data();
  e.num_hash_rows = hash_rows.size();
  e.ts_rows = ts_rows.data();
  e.num_ts_rows = ts_rows.size();
  e.hashes = hashes.data();
  e.num_hashes = hashes.size();
  e.total_hashes = rows.hashes;
  e.ts = ts.data();
  e.num_ts = ts.size();
  e.total_ts = rows.ts;
  e.seqs = rows.seqs.data();
  e.row_len = row_len.data();
  e.row_ts = rows.row_ts.data();
  e.hash_duration = hash_duration.data();
  e.problems = plan.problems.data();
  e.num_problems = plan.problems.size();
  e.pair_ids = plan.pair_ids.data();
  e.num_pairs = plan.pair_ids.size();
  IndexAppendOut out;
  Status s = gpu_index_edit(store_, e, &out);
  if (!s.ok()) return s;
  s = settle(cmp_, "Index::replace", R, (uint64_t)plan.pair_ids.size() * R, ids, [&](uint64_t l) { return plan.pair_ids[l]; }, row_seq, video,
             [&](const auto &...computed) { return gpu_index_edit_host_entries(store_, e, computed..., &out); }, out);
  if (!s.ok()) return s;
  // commit: nothing above changed the index
  index_store_switch(store_, e, out.held);
  std::vector<FrameHashesData> videos;
  std::vector<NeedleHipSearchResult> results(n1, NeedleHipSearchResult{});
  videos.reserve(n1);
  for (size_t v = 0; v < n1; v++) {
    if (is_fresh(v)) {
      videos.push_back(*fresh[v]);
    } else {
      videos.push_back(std::move(videos_[old_of_new[v]]));
      results[v] = results_[old_of_new[v]];
    }
  }
  for (size_t q = 0; q < out.videos.size(); q++) results[out.videos[q]] = out.results[q];
  videos_.swap(videos);
  results_.swap(results);
  labels_.swap(plan.labels);
  ids_ = std::move(plan.ids);
  rows_ = std::move(rows);
  changed(plan.searched, plan.searched);
  return Status::Ok();
}

Status Index::store_sizes(uint64_t sizes[4]) const { return index_store_sizes(store_, sizes); }

Status Index::evidence(NeedleHipSearchEvidence *out) const {
  if (!out) return Status::Make(NeedleError_NullArgument, "index evidence: null argument");
  if (videos_.empty()) return Status::Ok();
  IndexOptions o;
  set_options(cmp_, regions_, rows_.large_ok, *ids_, &o);
  return gpu_index_evidence(store_, o, out);
}

}  // namespace needle
