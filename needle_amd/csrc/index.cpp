// NeedleHipIndex: an incremental search index (include/needle_hip.h, "Incremental index"; DESIGN.md "Incremental index").
//
// find_best_match for video v (comparator.rs:405-515) is a pure function of v's candidate list: its pairs' heap entries in
// the reference's pair order, (q, v) for q < v, then (v, q) for q > v (:414-431, 534-545).  When videos are only APPENDED,
// every existing pair keeps its source / destination roles, and every new pair of an old video v is (v, new), after all
// of v's old pairs in the full search over the concatenated list.  So keeping every pair's entries, computing entries for
// the new pairs only and re-running best_match for the videos whose candidate list changed is bit-identical to
// Comparator::run_with_frame_hashes over all videos in insertion order.  The entries live on the device (epilogue.hip,
// IndexStore) under column-major pair ids p(i, j) = j (j - 1) / 2 + i, which do not depend on the number of videos.
#include "index.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "epilogue.h"

namespace needle {

Index::Index(const Comparator &comparator)
    : cmp_(comparator), include_endings_(comparator.include_endings()), regions_(comparator.include_endings() ? 2u : 1u) {}

Index::~Index() { index_store_free(store_); }

Status Index::init() {
  store_ = index_store_new();
  return Status::Ok();
}

Status Index::add(const std::vector<const FrameHashesData *> &fh) {
  if (fh.empty()) return Status::Make(NeedleError_InvalidArgument, "index add: no videos");
  const size_t k = fh.size(), n0 = videos_.size(), n1 = n0 + k, R = regions_;
  if (n1 >= 0xFFFFFFFFull) return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 videos");
  auto video = [&](size_t v) -> const FrameHashesData & { return v < n0 ? videos_[v] : *fh[v - n0]; };
  auto row_seq = [&](size_t v, size_t r) -> const std::vector<HashTs> & { return r == 0 ? video(v).opening : video(v).ending; };
  if (include_endings_ && n1 > 1)
    for (size_t v = 0; v < n1; v++)
      if (video(v).ending.empty())  // comparator.rs:271-273 (every video is in some pair)
        return Status::Make(NeedleError_Unknown, "no ending hash data present");
  // the new rows: hashes behind the arena's, timestamps behind the table's (a row whose timestamps equal video 0's of the
  // same region reads that table, as in run_with_frame_hashes' device epilogue)
  std::vector<NeedleHipSeq> seqs(seqs_);
  std::vector<uint32_t> min_len(min_len_), row_ts(row_ts_), new_row_len, new_row_ts, hashes;
  std::vector<uint64_t> ts, hash_duration;
  uint64_t num_hashes = hashes_, num_ts = ts_;
  bool large_ok = large_ok_;
  for (size_t v = n0; v < n1; v++) {
    hash_duration.push_back(video(v).hash_duration);
    for (size_t r = 0; r < R; r++) {
      const std::vector<HashTs> &seq = row_seq(v, r);
      if (num_hashes + seq.size() > UINT32_MAX)  // offsets into the arena are 32-bit on the device (NeedleHipSeq.offset)
        return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 hashes or sequence pairs");
      seqs.push_back(NeedleHipSeq{(uint32_t)num_hashes, (uint32_t)seq.size()});
      num_hashes += seq.size();
      for (const HashTs &h : seq) hashes.push_back(h.hash);
      min_len.push_back(cmp_.min_run_length_for(seq, r == 0));
      new_row_len.push_back((uint32_t)seq.size());
      const std::vector<HashTs> &first = row_seq(0, r);
      bool same = v > 0 && seq.size() == first.size();
      for (size_t q = 0; q < seq.size() && same; q++) same = seq[q].ts == first[q].ts;
      if (same) {
        row_ts.push_back(row_ts[r]);
      } else {
        row_ts.push_back((uint32_t)num_ts);
        for (const HashTs &h : seq) ts.push_back(h.ts);
        num_ts += seq.size();
        if (num_ts > UINT32_MAX) return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 timestamps");
      }
      new_row_ts.push_back(row_ts.back());
      large_ok = large_ok && seq.size() < 65536u;  // what pair_entries_large_kernel's packed keys stand on
      for (size_t q = 1; q < seq.size() && large_ok; q++) large_ok = seq[q].ts > seq[q - 1].ts;
    }
  }
  // the new pairs (i, j), j in [n0, n1), i < j, in column-major order; min_len and the pairs left out as in
  // run_with_frame_hashes (a pair one of whose sequences can hold no run long enough)
  const uint64_t first_pair = (uint64_t)n0 * (n0 ? n0 - 1 : 0) / 2;
  const uint64_t new_pairs = (uint64_t)n1 * (n1 - 1) / 2 - first_pair;
  if (((uint64_t)n1 * (n1 - 1) / 2) * R >= 0xFFFFFFF0ull)  // problem tags and bucket ids are 32-bit on the device
    return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 hashes or sequence pairs");
  std::vector<NeedleHipProblem> problems;
  problems.reserve(new_pairs * R);
  uint64_t searched = 0;
  for (size_t j = n0; j < n1; j++)
    for (size_t i = 0; i < j; i++) {
      const uint64_t rel = (uint64_t)j * (j - 1) / 2 + i - first_pair;
      bool any = false;
      for (size_t r = 0; r < R; r++) {
        const uint32_t a = min_len[i * R + r], b = min_len[j * R + r];
        if (a == 0 || b == 0) continue;
        problems.push_back(NeedleHipProblem{(uint32_t)(i * R + r), (uint32_t)(j * R + r), std::max(a, b), (uint32_t)(rel * R + r)});
        any = true;
      }
      searched += any;
    }
  IndexAppend a;
  a.n0 = (uint32_t)n0;
  a.n1 = (uint32_t)n1;
  a.regions = (uint32_t)R;
  a.threshold = cmp_.hash_match_threshold();
  a.include_endings = include_endings_;
  a.large_ok = large_ok;
  a.min_opening_duration = cmp_.min_opening_duration();
  a.min_ending_duration = cmp_.min_ending_duration();
  a.time_padding = cmp_.time_padding();
  a.hashes = hashes.data();
  a.num_hashes = hashes.size();
  a.seqs = seqs.data();
  a.num_seqs = seqs.size();
  a.problems = problems.data();
  a.num_problems = problems.size();
  a.row_len = new_row_len.data();
  a.row_ts = new_row_ts.data();
  a.num_rows = new_row_len.size();
  a.ts = ts.data();
  a.num_ts = ts.size();
  a.hash_duration = hash_duration.data();
  IndexAppendOut out;
  Status s = gpu_index_append(store_, a, &out);
  if (!s.ok()) return s;
  if (out.failed & kEpilogueBucketTooLarge) {
    // A bucket the device does not order (beyond kEpilogueLargeLimit runs, or rows the packed keys cannot stand for): this
    // append's new-pair entries are computed here from its run list, with the host form's own functions.
    note_epilogue_host_fallback("Index::add", out.runs.size(), n1);
    const uint64_t buckets = new_pairs * R;
    std::vector<uint32_t> start(buckets + 1, 0), valid(buckets, 0);
    for (const NeedleHipRun &r : out.runs)
      if (r.problem < buckets) start[r.problem + 1]++;
    for (uint64_t b = 0; b < buckets; b++) start[b + 1] += start[b];
    std::vector<NeedleHipRun> sorted(start[buckets]);
    {
      std::vector<uint32_t> fill(start.begin(), start.end() - 1);
      for (const NeedleHipRun &r : out.runs)
        if (r.problem < buckets) sorted[fill[r.problem]++] = r;
    }
    std::vector<IndexEntry> entries(out.runs.size());
    std::vector<HeapEntry> tmp;
    for (uint64_t b = 0; b < buckets; b++) {
      const uint32_t lo = start[b], hi = start[b + 1];
      if (hi == lo) continue;
      std::sort(sorted.begin() + lo, sorted.begin() + hi, [](const NeedleHipRun &x, const NeedleHipRun &y) {
        return x.src_end != y.src_end ? x.src_end > y.src_end : x.dst_end > y.dst_end;  // the reference's walk (:191-192)
      });
      const uint64_t p = first_pair + b / R;
      const size_t r = b % R;
      size_t j = (size_t)((1.0 + std::sqrt(1.0 + 8.0 * (double)p)) / 2.0);
      while (j > 1 && (uint64_t)j * (j - 1) / 2 > p) j--;
      while ((uint64_t)(j + 1) * j / 2 <= p) j++;
      const size_t i = (size_t)(p - (uint64_t)j * (j - 1) / 2);
      cmp_.entries_from_runs(&sorted[lo], hi - lo, row_seq(i, r), row_seq(j, r), video(i).hash_duration, video(j).hash_duration,
                             r == 0, &tmp);
      for (size_t q = 0; q < tmp.size(); q++) {
        const HeapEntry &e = tmp[q];
        entries[lo + q] = IndexEntry{e.src_start, e.src_end, e.dst_start, e.dst_end, (uint32_t)e.score, e.src_match_hash, e.dst_match_hash, 0u};
      }
      valid[b] = (uint32_t)tmp.size();
    }
    start.pop_back();
    if (!(s = gpu_index_append_host_entries(store_, a, start, valid, entries, &out)).ok()) return s;
  }
  if (out.failed)  // best_match_kernel: the winner's end minus padding / hash duration underflows (the reference panics)
    return Status::Make(NeedleError_Unknown, "overflow when subtracting durations (time_padding / hash_duration exceed the match end)");
  // commit: nothing above changed the index
  index_store_commit(store_, a, out.found);
  for (const FrameHashesData *d : fh) videos_.push_back(*d);
  seqs_.swap(seqs);
  min_len_.swap(min_len);
  row_ts_.swap(row_ts);
  hashes_ = num_hashes;
  ts_ = num_ts;
  large_ok_ = large_ok;
  results_.resize(n1, NeedleHipSearchResult{});
  for (size_t q = 0; q < out.videos.size(); q++) results_[out.videos[q]] = out.results[q];
  pairs_last_ = searched;
  pairs_total_ += searched;
  return Status::Ok();
}

}  // namespace needle
