// meduce-gpu: drop-in CLI for the reference binary (/root/reference/src/main.rs).
// Same input default ("shakes.txt" in the working directory, main.rs:10), same
// outputs: final_result.txt with "{word} {count}\n" lines (main.rs:170-182) and
// "Top 10 words:" + "{word}: {count}" on stdout (main.rs:184-192).  The hot
// section (main.rs:16-22) is one mox_run_file call on the GPU; the file's text
// is rendered there too (mox_write_result) and the ten words are selected there
// (mox_top_words), so the table itself never reaches the host.  No
// intermediate map files exist, so the reference's cleanup lines
// ("Successfully deleted: ...", main.rs:194-202) are not printed.
// Beyond the reference: every positional argument is an input file, counted
// together (separate corpora: no token runs from one file into the next), and
// --chunk BYTES reads each file in passes of about BYTES cut at whitespace, so
// that neither one file nor all of them need fit in device memory.  Both go
// through the device-resident accumulator (mox_accumulate_file); one file
// without --chunk is the single mox_run_file call it always was.
// --word W (repeatable) prints, after the top-10 block, "Counts:" and one
// "{word}: {count}" line per W in argument order, read from the device-resident
// result (mox_lookup_words).  W is taken verbatim: the table holds lowercased
// words, so "The" counts 0.  Without --word the output is what it always was.
// --min-count N and --stop FILE apply one filter to the device-resident result
// (mox_filter_result) after counting and before the file, the top ten and
// --word: words seen fewer than N times and the words of FILE go.  FILE holds
// words split at ASCII whitespace, taken verbatim (lowercase them: the table's
// words are).  Without these options the output is what it always was.
// --by-count orders the device-resident result by count, most frequent first,
// words with equal counts bytewise (mox_sort_result, then the stable
// mox_rank_result), after any filter and before the file is written:
// final_result.txt is then the same from run to run.  Without the option
// every output is what it always was.
// --trim-punct re-keys the total on the device (mox_rekey_result with
// MOX_REKEY_TRIM_ASCII_PUNCT): ASCII punctuation is stripped from both ends of
// every word and the variants are summed ("the," and "(the)" count as "the"),
// words of punctuation alone go.  It applies before --min-count, --stop and
// --by-count, and before anything is written or printed.  Without the option
// every output is what it always was.
// --prefix P (repeatable) prints, after everything else, "Prefix {P}: {rows}
// words, {tokens} tokens" and up to ten "{word}: {count}" lines, the most
// frequent words that start with P: the result is put in bytewise order on the
// device if it is not (mox_sort_result; final_result.txt is then in that order
// too, unless --by-count ranks it), two binary searches give P's row range and
// the sum of its counts (mox_find_ranges) and the ten words are selected from
// those rows alone (mox_top_rows).  The queries run after that sort and before
// any --by-count ranking.  P is taken verbatim, as --word's W.  Without the
// option every output is what it always was.
// --not-in BASE keeps only the input's words that the file BASE lacks (the new
// words), --also-in BASE only those BASE holds too, each with the input's own
// count (mox_join_total): BASE is counted into the device-resident accumulator
// first, re-keyed first when --trim-punct is given, then the single input file
// is counted and joined against that total on the device, after --trim-punct
// and before --min-count, --stop and --by-count apply.  The tool's own
// multi-file total uses the accumulator, so more than one input file, or
// --chunk, together with either option is a usage error, and so are both
// options together: exit status 2.  Without the options every output is what
// it always was.
// --histogram KEY (repeatable; KEY is count, bytes, chars or first; anything
// else is a usage error: exit status 2) prints, after everything else,
// "Histogram {KEY}: {bins} bins, {words} words, {tokens} tokens" and one
// "{key}\t{words}\t{tokens}" line per bin, keys ascending: the words and tokens
// per count (the frequency spectrum), per word length in bytes or characters,
// or per first character, binned on the device (mox_hist_result).  The key is
// in decimal; for first it is the character's bytes.  The histogram is read
// from the result as it stands at that point, after any filter, re-key or
// ranking.  Without the option every output is what it always was.
// Exit status 1 with a message on stderr on any error, like `main` returning Err.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "mox.h"

int main(int argc, char** argv) {
  std::vector<std::string> paths;
  std::string out = "final_result.txt";
  int device = -1;
  unsigned long long chunk = 0;
  std::vector<std::string> words, prefixes, hists;
  unsigned long long min_count = 0;
  std::string stop_path, base_path;
  int n_not_in = 0, n_also_in = 0;
  bool have_stop = false, by_count = false, trim_punct = false;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--out") && i + 1 < argc) out = argv[++i];
    else if (!strcmp(argv[i], "--chunk") && i + 1 < argc) chunk = strtoull(argv[++i], nullptr, 10);
    else if (!strcmp(argv[i], "--word") && i + 1 < argc) words.push_back(argv[++i]);
    else if (!strcmp(argv[i], "--prefix") && i + 1 < argc) prefixes.push_back(argv[++i]);
    else if (!strcmp(argv[i], "--histogram") && i + 1 < argc) hists.push_back(argv[++i]);
    else if (!strcmp(argv[i], "--min-count") && i + 1 < argc) min_count = strtoull(argv[++i], nullptr, 10);
    else if (!strcmp(argv[i], "--stop") && i + 1 < argc) { stop_path = argv[++i]; have_stop = true; }
    else if (!strcmp(argv[i], "--not-in") && i + 1 < argc) { base_path = argv[++i]; n_not_in++; }
    else if (!strcmp(argv[i], "--also-in") && i + 1 < argc) { base_path = argv[++i]; n_also_in++; }
    else if (!strcmp(argv[i], "--by-count")) by_count = true;
    else if (!strcmp(argv[i], "--trim-punct")) trim_punct = true;
    else paths.push_back(argv[i]);
  }
  if (paths.empty()) paths.push_back("shakes.txt");
  const char* const hist_names[4] = {"count", "bytes", "chars", "first"};  // MOX_HIST_COUNT .. MOX_HIST_FIRST
  std::vector<uint32_t> hist_keys;
  for (const std::string& k : hists) {
    uint32_t key = 0;
    while (key < 4 && k != hist_names[key]) key++;
    if (key == 4) { fprintf(stderr, "Usage: --histogram count|bytes|chars|first\n"); return 2; }
    hist_keys.push_back(key);
  }
  const bool join = n_not_in || n_also_in;
  if (n_not_in && n_also_in) { fprintf(stderr, "Usage: --not-in and --also-in exclude each other\n"); return 2; }
  if (n_not_in + n_also_in > 1) { fprintf(stderr, "Usage: one --not-in or --also-in\n"); return 2; }
  if (join && (paths.size() > 1 || chunk)) {
    fprintf(stderr, "Usage: --not-in / --also-in take one input file and no --chunk (the accumulator holds BASE)\n");
    return 2;
  }
  // the stop list: the file's words, split at ASCII whitespace
  std::string stop_bytes;
  std::vector<uint64_t> stop_offs(1, 0);
  if (have_stop) {
    std::ifstream in(stop_path, std::ios::binary);
    if (!in) { fprintf(stderr, "Error: cannot open %s\n", stop_path.c_str()); return 1; }
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    auto is_ws = [](unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); };
    for (size_t i = 0; i < text.size();) {
      while (i < text.size() && is_ws((unsigned char)text[i])) i++;
      size_t j = i;
      while (j < text.size() && !is_ws((unsigned char)text[j])) j++;
      if (j > i) {
        stop_bytes.append(text, i, j - i);
        stop_offs.push_back(stop_bytes.size());
      }
      i = j;
    }
  }
  mox_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.device = device;
  mox_engine* e = nullptr;
  if (mox_engine_create(&cfg, &e) != MOX_OK) { fprintf(stderr, "Error: %s\n", mox_last_error()); return 1; }
  mox_table* t = nullptr;
  int rc = MOX_OK;
  mox_rekey rk;
  memset(&rk, 0, sizeof rk);
  rk.flags = MOX_REKEY_TRIM_ASCII_PUNCT;
  if (join) {  // BASE becomes the accumulator's total
    rc = mox_run_file(e, base_path.c_str());
    if (rc == MOX_OK && trim_punct) rc = mox_rekey_result(e, &rk, nullptr);
    if (rc == MOX_OK) rc = mox_accumulate(e);
  }
  if (paths.size() == 1 && !chunk) {
    if (rc == MOX_OK) rc = mox_run_file(e, paths[0].c_str());
  } else {
    for (size_t i = 0; i < paths.size() && rc == MOX_OK; i++) rc = mox_accumulate_file(e, paths[i].c_str(), chunk);
  }
  if (rc == MOX_OK && trim_punct) rc = mox_rekey_result(e, &rk, nullptr);
  if (rc == MOX_OK && join) {
    mox_join j;
    memset(&j, 0, sizeof j);
    j.mode = n_not_in ? MOX_JOIN_ANTI : MOX_JOIN_SEMI;
    rc = mox_join_total(e, &j, nullptr);
  }
  if (rc == MOX_OK && (min_count || have_stop)) {
    mox_filter f;
    memset(&f, 0, sizeof f);
    f.min_count = min_count;
    f.words = (const uint8_t*)stop_bytes.data();
    f.word_offs = stop_offs.data();
    f.n_words = stop_offs.size() - 1;
    f.words_mode = MOX_FILTER_WORDS_DROP;
    rc = mox_filter_result(e, &f, nullptr);
  }
  if (rc == MOX_OK && (by_count || !prefixes.empty())) rc = mox_sort_result(e);
  // the prefix queries, on the sorted table: the ranges, their tokens and their ten words (printed last)
  std::vector<uint64_t> p_first(prefixes.size()), p_last(prefixes.size()), p_sums(prefixes.size());
  std::vector<mox_table*> p_top(prefixes.size(), nullptr);
  if (rc == MOX_OK && !prefixes.empty()) {
    std::string bytes;
    std::vector<uint64_t> offs(1, 0);
    for (const std::string& p : prefixes) {
      bytes += p;
      offs.push_back(bytes.size());
    }
    rc = mox_find_ranges(e, (const uint8_t*)bytes.data(), offs.data(), prefixes.size(), MOX_FIND_PREFIX, p_first.data(), p_last.data(),
                         p_sums.data(), nullptr);
    for (size_t i = 0; i < prefixes.size() && rc == MOX_OK; i++) rc = mox_top_rows(e, p_first[i], p_last[i] - p_first[i], 10, &p_top[i]);
  }
  if (rc == MOX_OK && by_count) rc = mox_rank_result(e, 0, nullptr);
  if (rc == MOX_OK) rc = mox_write_result(e, out.c_str());
  if (rc == MOX_OK) rc = mox_top_words(e, 10, &t);
  if (rc == MOX_OK) rc = mox_print_top_words(t, 10);
  if (rc == MOX_OK && !words.empty()) {
    std::string bytes;
    std::vector<uint64_t> offs(1, 0), counts(words.size());
    for (const std::string& w : words) {
      bytes += w;
      offs.push_back(bytes.size());
    }
    rc = mox_lookup_words(e, (const uint8_t*)bytes.data(), offs.data(), words.size(), counts.data(), nullptr, nullptr);
    if (rc == MOX_OK) {
      printf("Counts:\n");
      for (size_t i = 0; i < words.size(); i++) printf("%s: %llu\n", words[i].c_str(), (unsigned long long)counts[i]);
    }
  }
  for (size_t i = 0; i < prefixes.size() && rc == MOX_OK; i++) {
    printf("Prefix %s: %llu words, %llu tokens\n", prefixes[i].c_str(), (unsigned long long)(p_last[i] - p_first[i]),
           (unsigned long long)p_sums[i]);
    const mox_table* pt = p_top[i];
    for (uint64_t j = 0; j < pt->n; j++) {
      fwrite(pt->bytes + pt->offs[j], 1, pt->offs[j + 1] - pt->offs[j], stdout);
      printf(": %llu\n", (unsigned long long)pt->counts[j]);
    }
  }
  for (size_t i = 0; i < hist_keys.size() && rc == MOX_OK; i++) {
    mox_hist h;
    memset(&h, 0, sizeof h);
    h.key = hist_keys[i];
    mox_hist_table* ht = nullptr;
    rc = mox_hist_result(e, &h, &ht, nullptr);
    if (rc != MOX_OK) break;
    printf("Histogram %s: %llu bins, %llu words, %llu tokens\n", hists[i].c_str(), (unsigned long long)ht->n, (unsigned long long)ht->words,
           (unsigned long long)ht->tokens);
    for (uint64_t b = 0; b < ht->n; b++) {
      if (h.key == MOX_HIST_FIRST) {
        for (uint64_t x = 0; x < (ht->keys[b] & 0xFF); x++) putchar((int)((ht->keys[b] >> (32 - 8 * x)) & 0xFF));
      } else {
        printf("%llu", (unsigned long long)ht->keys[b]);
      }
      printf("\t%llu\t%llu\n", (unsigned long long)ht->bin_words[b], (unsigned long long)ht->bin_tokens[b]);
    }
    mox_hist_free(ht);
  }
  if (rc != MOX_OK) fprintf(stderr, "Error: %s\n", mox_last_error());
  for (mox_table* pt : p_top) mox_table_free(pt);
  mox_table_free(t);
  mox_engine_destroy(e);
  return rc == MOX_OK ? 0 : 1;
}
