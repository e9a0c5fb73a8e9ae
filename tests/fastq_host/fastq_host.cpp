// fastq_host.cpp -- csrc/bpsw_fastq_core.h (the record rules and parse_serial, what BPSW_FASTQ_HOST runs and what the kernels of
// bpsw_fastq.hip call per read) compiled for the host under -fsanitize=address,undefined, against
//   1. the cases file given as argv[1]: texts with the fields the reference's bseq_read returned for them (written by
//      tests/test_fastq_core_host.py from tests/golden/fastq_cases.npz);
//   2. a few thousand generated records with random line ends, name shapes, comments and lengths -- single texts, two texts and
//      interleaved ones, whole, cut at a random byte, with one record broken -- against the fields the generator itself wrote down and
//      an independent line splitter (memchr, std::string) that shares nothing with the header.
// Every output array is allocated at exactly the size `needed` reports, so a store past it is the sanitizer's to find.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "bpsw_fastq_core.h"

namespace fq = bpsw::fqcore;

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
      exit(1);                                             \
    }                                                      \
  } while (0)

struct Parsed {
  int how = 0;
  fq::Result res{};
  std::vector<int32_t> read_len;
  std::vector<int64_t> read_off, name_off;
  std::vector<uint8_t> read_pool, qual_pool;
  std::vector<char> name_pool;
};

static Parsed run(const std::string& t1, const std::string* t2, int flags) {
  Parsed P;
  // exact copies on the heap: a read past a text's end is the sanitizer's to find
  std::vector<char> a(t1.begin(), t1.end()), b;
  if (t2) b.assign(t2->begin(), t2->end());
  static char nothing[1];
  const char* text[2] = {a.empty() ? nothing : a.data(), t2 ? (b.empty() ? nothing : b.data()) : nullptr};
  const long long bytes[2] = {(long long)a.size(), (long long)b.size()};
  auto room = [&](const fq::Result& r, fq::Outputs* o) {
    const bool pairs = t2 || (flags & fq::PAIR_NAMES);
    P.read_len.resize((size_t)r.needed[0]); P.read_off.resize((size_t)r.needed[0]);
    P.name_off.resize((size_t)(pairs ? r.needed[0] / 2 : r.needed[0]) + 1);
    P.read_pool.resize((size_t)r.needed[1]); P.qual_pool.resize((size_t)r.needed[1]); P.name_pool.resize((size_t)r.needed[2]);
    o->read_len = P.read_len.data(); o->read_off = P.read_off.data(); o->read_pool = P.read_pool.data(); o->qual_pool = P.qual_pool.data();
    o->name_off = P.name_off.data(); o->name_pool = P.name_pool.data();
    return true;
  };
  P.how = fq::parse_serial(text, bytes, t2 ? 2 : 1, flags, room, &P.res);
  return P;
}

// ---- what is expected, as plain fields -----------------------------------------------------------------------------------------------
struct Fields {
  std::string name, seq, qual;
};
static int code_of(unsigned char c) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
  }
}
static void expect_reads(const Parsed& P, const std::vector<Fields>& want, bool pairs, const char* what) {
  CHECK(P.how == fq::PARSE_OK, "%s: how %d, read %lld reason %d", what, P.how, P.res.bad_read, P.res.bad_reason);
  CHECK(P.res.n_reads == (long long)want.size(), "%s: %lld reads, expected %zu", what, P.res.n_reads, want.size());
  long long at = 0, name_at = 0;
  size_t k = 0;
  for (size_t i = 0; i < want.size(); ++i) {
    const Fields& f = want[i];
    CHECK(P.read_len[i] == (int32_t)f.seq.size() && P.read_off[i] == at, "%s: read %zu: len %d off %lld", what, i, P.read_len[i], (long long)P.read_off[i]);
    for (size_t j = 0; j < f.seq.size(); ++j) {
      CHECK(P.read_pool[(size_t)at + j] == code_of((unsigned char)f.seq[j]), "%s: read %zu base %zu", what, i, j);
      CHECK(P.qual_pool[(size_t)at + j] == (uint8_t)f.qual[j], "%s: read %zu quality %zu", what, i, j);
    }
    at += (long long)f.seq.size();
    if (pairs && (i & 1)) continue;
    CHECK(P.name_off[k] == name_at, "%s: name %zu at %lld", what, k, (long long)P.name_off[k]);
    CHECK(std::string(P.name_pool.data() + name_at, f.name.size()) == f.name, "%s: name %zu", what, k);
    name_at += (long long)f.name.size();
    ++k;
  }
  CHECK(P.name_off[k] == name_at && P.res.needed[1] == at && P.res.needed[2] == name_at, "%s: totals", what);
}

// ---- the independent splitter --------------------------------------------------------------------------------------------------------
// the whole records of a text as fields: lines by memchr, groups of four; *consumed: the offset behind the last whole record
static std::vector<Fields> split_text(const std::string& t, bool final, long long* consumed, bool* leftover) {
  std::vector<std::string> lines;
  std::vector<size_t> ends;
  size_t at = 0;
  while (at < t.size()) {
    const void* nl = memchr(t.data() + at, '\n', t.size() - at);
    if (!nl) {
      if (final) { lines.push_back(t.substr(at)); ends.push_back(t.size()); }
      break;
    }
    const size_t e = (size_t)((const char*)nl - t.data());
    lines.push_back(t.substr(at, e - at));
    ends.push_back(e + 1);
    at = e + 1;
  }
  std::vector<Fields> out;
  for (size_t r = 0; r + 4 <= lines.size(); r += 4) {
    Fields f;
    std::string h = lines[r].substr(1), s = lines[r + 1], q = lines[r + 3];
    const size_t sp = h.find_first_of(" \t\v\f\r");
    f.name = h.substr(0, sp);
    if (f.name.size() > 2 && f.name[f.name.size() - 2] == '/' && isdigit((unsigned char)f.name.back())) f.name.resize(f.name.size() - 2);
    if (s.size() > 1 && s.back() == '\r') s.pop_back();
    if (q.size() > 1 && q.back() == '\r') q.pop_back();
    f.seq = s; f.qual = q;
    out.push_back(f);
  }
  *consumed = out.empty() ? 0 : (long long)ends[4 * out.size() - 1];
  *leftover = lines.size() % 4 != 0;
  return out;
}

// ---- 1. the recorded cases -------------------------------------------------------------------------------------------------------------
static std::string get_bytes(FILE* f) {
  long long n = 0;
  CHECK(fread(&n, 8, 1, f) == 1 && n >= 0, "cases file: a length");
  std::string s((size_t)n, '\0');
  CHECK(n == 0 || fread(&s[0], 1, (size_t)n, f) == (size_t)n, "cases file: bytes");
  return s;
}
static long long get_i64(FILE* f) {
  long long v = 0;
  CHECK(fread(&v, 8, 1, f) == 1, "cases file: a number");
  return v;
}

static int recorded_cases(const char* path) {
  FILE* f = fopen(path, "rb");
  CHECK(f, "cannot open %s", path);
  const long long n_cases = get_i64(f);
  long long reads = 0;
  for (long long c = 0; c < n_cases; ++c) {
    const std::string name = get_bytes(f);
    const int flags = (int)get_i64(f);
    const bool two = get_i64(f) != 0;
    const long long stops_at = get_i64(f);  // >= 0: the text is refused, at this record
    const std::string t1 = get_bytes(f), t2 = get_bytes(f);
    const long long n = get_i64(f);
    std::vector<Fields> want((size_t)n);
    for (auto& w : want) { w.name = get_bytes(f); w.seq = get_bytes(f); w.qual = get_bytes(f); }
    const Parsed P = run(t1, two ? &t2 : nullptr, flags);
    if (stops_at >= 0) {
      CHECK(P.how == fq::PARSE_BAD && P.res.bad_read == stops_at, "%s: how %d, bad read %lld, the reference stops at %lld", name.c_str(), P.how,
            P.res.bad_read, stops_at);
      continue;
    }
    expect_reads(P, want, two || (flags & fq::PAIR_NAMES), name.c_str());
    reads += n;
  }
  fclose(f);
  printf("fastq core: %lld recorded cases, %lld reads: equal\n", n_cases, reads);
  return 0;
}

// ---- 2. generated records ----------------------------------------------------------------------------------------------------------------
struct Gen {
  std::mt19937_64 rng{20240612};
  int pick(int n) { return (int)(rng() % (unsigned long long)n); }
  std::string letters(int n, const char* from) {
    std::string s;
    const int k = (int)strlen(from);
    for (int i = 0; i < n; ++i) s.push_back(from[pick(k)]);
    return s;
  }
  // a record's text and the fields it stands for; suffix: what follows the name's stem ("" or "/1", "/2")
  std::string record(const std::string& stem, const std::string& suffix, Fields* f) {
    static const char* shapes[] = {"", "/", "/x", "/a/b", ".7", "_"};
    f->name = stem + shapes[pick(6)];
    if (f->name.size() > 2 && f->name[f->name.size() - 2] == '/' && isdigit((unsigned char)f->name.back())) f->name += "_";
    std::string full = f->name + suffix;
    if (suffix.empty() && pick(5) == 0) { full += "/" + std::to_string(pick(10)); }  // (trimmed away again)
    const char* seps[] = {" ", "\t", "\v", "\f"};
    std::string header = "@" + full;
    if (pick(3) == 0) header += std::string(seps[pick(4)]) + letters(pick(40), "abc /@+1");
    const int len = pick(12) == 0 ? 1 + pick(300) : 1 + pick(60);
    f->seq = letters(len, "ACGTacgtNnRYKM.*");
    f->qual = letters(len, "!\"#$%&'()*+,-./0123456789:;<=>?@ABCDEFGHIJ");
    const std::string eol = pick(4) == 0 ? "\r\n" : "\n";
    std::string plus = "+";
    if (pick(4) == 0) plus += full;
    return header + eol + f->seq + eol + plus + eol + f->qual + eol;
  }
};

static int generated() {
  Gen G;
  long long records = 0, texts = 0, cut_texts = 0, refused = 0, pair_texts = 0;
  for (int round = 0; round < 400; ++round) {
    const int mode = round % 4;  // 0, 1: one text; 2: two texts; 3: interleaved with one name per pair
    const int n = G.pick(24);
    std::vector<Fields> want;
    std::string t1, t2;
    for (int k = 0; k < n; ++k) {
      Fields f;
      const std::string stem = "r" + std::to_string(round) + "_" + std::to_string(k);
      if (mode < 2) { t1 += G.record(stem, "", &f); want.push_back(f); continue; }
      const std::string first = G.record(stem, G.pick(2) ? "/1" : "", &f);
      const std::string name = f.name;
      want.push_back(f);
      std::string second;
      do { second = G.record(stem, G.pick(2) ? "/2" : "", &f); } while (f.name != name);  // (the shapes are drawn again until they agree)
      want.push_back(f);
      if (mode == 2) { t1 += first; t2 += second; }
      else t1 += first + second;
    }
    const bool pairs = mode >= 2;
    const int flags = mode == 3 ? fq::INTERLEAVED | fq::PAIR_NAMES : 0;
    // whole, with FINAL: every record, everything consumed
    {
      const Parsed P = run(t1, mode == 2 ? &t2 : nullptr, flags | fq::FINAL);
      expect_reads(P, want, pairs, "generated, whole");
      CHECK(P.res.consumed[0] == (long long)t1.size() && P.res.consumed[1] == (long long)t2.size(), "generated, whole: consumed");
      long long c = 0;
      bool left = false;
      const std::vector<Fields> again = split_text(t1, true, &c, &left);
      if (mode != 2) {
        CHECK(again.size() == want.size() && !left && c == (long long)t1.size(), "the splitter and the generator disagree");
        for (size_t i = 0; i < want.size(); ++i)
          CHECK(again[i].seq == want[i].seq && again[i].qual == want[i].qual && again[i].name == want[i].name, "the splitter and the generator disagree at %zu", i);
      }
      records += (long long)want.size();
      ++texts;
      pair_texts += pairs;
    }
    if (t1.empty()) continue;
    // cut at a random byte, without FINAL: the whole records before the cut, and where they end (the splitter's word)
    if (mode < 2) {
      const size_t cut = (size_t)G.pick((int)t1.size() + 1);
      const std::string part = t1.substr(0, cut);
      long long c = 0;
      bool left = false;
      const std::vector<Fields> head = split_text(part, false, &c, &left);
      const Parsed P = run(part, nullptr, 0);
      expect_reads(P, head, false, "generated, cut");
      CHECK(P.res.consumed[0] == c, "generated, cut at %zu: consumed %lld, the splitter says %lld", cut, P.res.consumed[0], c);
      // ... and under FINAL the same cut either parses (the splitter then has no line left over and equal lengths) or is refused
      const std::vector<Fields> fin = split_text(part, true, &c, &left);
      const Parsed F = run(part, nullptr, fq::FINAL);
      bool ok = !left;
      for (const Fields& f : fin) ok = ok && f.seq.size() == f.qual.size() && !f.seq.empty();
      CHECK((F.how == fq::PARSE_OK) == ok, "generated, cut at %zu under FINAL: how %d, the splitter says %d", cut, F.how, (int)ok);
      if (ok) expect_reads(F, fin, false, "generated, cut, final");
      ++cut_texts;
    }
    // one record broken: refused at that read for that reason
    if (mode < 2 && n > 0) {
      const int bad = G.pick(n);
      long long c = 0;
      bool left = false;
      std::vector<Fields> all = split_text(t1, true, &c, &left);
      std::string t;
      const int kind = G.pick(6);
      static const int reason[] = {fq::R_NO_AT, fq::R_NO_PLUS, fq::R_LEN_DIFF, fq::R_DASH, fq::R_LOW_BYTE, fq::R_EMPTY_NAME};
      for (int k = 0; k < n; ++k) {
        const Fields& f = all[(size_t)k];
        std::string h = "@" + f.name + "x", s = f.seq, p = "+", q = f.qual;
        if (k == bad) {
          if (kind == 0) h[0] = '>';
          if (kind == 1) p = "-";
          if (kind == 2) q += "I";
          if (kind == 3) s[s.size() / 2] = '-';
          if (kind == 4) s[s.size() - 1] = (char)G.pick(4);
          if (kind == 5) h = "@ " + f.name;
        }
        t += h + "\n" + s + "\n" + p + "\n" + q + "\n";
      }
      const Parsed P = run(t, nullptr, fq::FINAL);
      CHECK(P.how == fq::PARSE_BAD && P.res.bad_read == bad && P.res.bad_reason == reason[kind], "generated, broken %d at %d: how %d read %lld reason %d",
            kind, bad, P.how, P.res.bad_read, P.res.bad_reason);
      ++refused;
    }
  }
  printf("fastq core: %lld generated records in %lld texts (%lld of pairs), %lld cut, %lld refused: equal\n", records, texts, pair_texts, cut_texts, refused);
  return 0;
}

int main(int argc, char** argv) {
  CHECK(argc == 2, "usage: fastq_host <cases file>");
  return recorded_cases(argv[1]) || generated();
}
