// The host side of predict mode's classification (reference utils/preprocess_featureFiles.py and utils/model_predict.py;
// the rule: tests/predict_model_model.py), no GPU: the reader of the screened table with the reference's three filter files
// (`<tmp>.csv`, `<tmp>_refined_tmp.csv`, `<tmp>_refined_features.csv`, byte for byte), the feature matrix pandas' read_csv
// and get_dummies lead to, and the two result files from the device's arrays.  The filters work on text exactly as the
// reference does: every file is made from the lines of the one before, stripped and split again.  Where this differs from
// the reference: lines end at '\n' alone (Python's text mode also ends one at a lone '\r'), and the three name cells are
// copied as text (pandas prints a name column of numbers as numbers, quotes cells again and empties NA markers).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "host_write.hpp"
#include "predict_svm.hpp"

namespace mrg {

namespace {

// what Python's str.strip() takes for white space in ASCII text
inline bool is_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= '\x1c' && c <= '\x1f'); }

std::string stripped(const char* p, size_t n) {
  while (n && is_space(p[0])) ++p, --n;
  while (n && is_space(p[n - 1])) --n;
  return std::string(p, n);
}
// str.split(sep): empty cells stay
std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  size_t at = 0;
  for (;;) {
    const size_t e = s.find(sep, at);
    if (e == std::string::npos) break;
    out.emplace_back(s, at, e - at);
    at = e + 1;
  }
  out.emplace_back(s, at);
  return out;
}
// the lines of a text as readline() gives them, stripped
std::vector<std::string> stripped_lines(const std::string& text) {
  std::vector<std::string> out;
  size_t at = 0;
  while (at < text.size()) {
    const void* nl = std::memchr(text.data() + at, '\n', text.size() - at);
    const size_t end = nl ? (size_t)(static_cast<const char*>(nl) - text.data()) + 1 : text.size();
    out.push_back(stripped(text.data() + at, end - at));
    at = end;
  }
  return out;
}
std::string joined(const std::vector<std::string>& cells, const std::vector<size_t>& which) {
  std::string out;
  bool first = true;
  for (size_t i : which) {
    if (i >= cells.size()) break;   // (which ascends)
    if (!first) out.push_back(',');
    out += cells[i];
    first = false;
  }
  return out;
}
size_t index_of(const std::vector<std::string>& cells, const char* name, const char* where) {
  for (size_t i = 0; i < cells.size(); ++i)
    if (cells[i] == name) return i;
  throw std::invalid_argument(std::string(where) + ": no column " + name);
}
// Python's int() of a count cell: an optional sign and digits; anything else is the reference's ValueError
long long count_of(const std::vector<std::string>& cells, size_t i, uint64_t line) {
  if (i < cells.size()) {
    const std::string t = stripped(cells[i].data(), cells[i].size());
    size_t k = (t.size() && (t[0] == '+' || t[0] == '-')) ? 1 : 0;
    bool ok = t.size() > k && t.size() - k <= 18;
    for (size_t j = k; ok && j < t.size(); ++j) ok = t[j] >= '0' && t[j] <= '9';
    if (ok) return std::atoll(t.c_str());
  }
  throw std::invalid_argument("line " + std::to_string(line) + " of the table: readCountSum or seqCount is no whole number");
}
// a cell of a column of numbers: digits, signs, a point and an exponent, read by strtod; everything else is text
bool number_of(const std::string& cell, double* v) {
  const std::string t = stripped(cell.data(), cell.size());
  if (t.empty() || t.size() > 64) return false;
  for (char c : t)
    if (!((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E')) return false;
  char* end = nullptr;
  *v = std::strtod(t.c_str(), &end);
  return end == t.c_str() + t.size();
}
std::vector<std::string> names_of(const char* text) {
  std::vector<std::string> out;
  for (std::string& s : stripped_lines(text ? text : "")) out.push_back(std::move(s));
  return out;
}

}  // namespace

void append_repr(std::string& out, double v) {
  if (std::isnan(v)) {
    out += "nan";
    return;
  }
  if (std::isinf(v)) {
    out += v < 0 ? "-inf" : "inf";
    return;
  }
  if (v == 0.0) {
    out += std::signbit(v) ? "-0.0" : "0.0";
    return;
  }
  // the shortest digits that read back as v: the correctly rounded p-digit form for the least p that does
  char buf[40];
  for (int p = 1; p <= 17; ++p) {
    std::snprintf(buf, sizeof buf, "%.*e", p - 1, v);
    if (std::strtod(buf, nullptr) == v) break;
  }
  const char* s = buf;
  if (*s == '-') out.push_back(*s++);
  std::string digits;
  digits.push_back(*s++);
  if (*s == '.') ++s;
  while (*s != 'e') digits.push_back(*s++);
  const int e10 = std::atoi(s + 1);
  while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
  const int nd = (int)digits.size(), decpt = e10 + 1;   // v = 0.digits * 10^decpt
  if (decpt <= -4 || decpt > 16) {   // float_repr_style 'short', format code 'r'
    out.push_back(digits[0]);
    if (nd > 1) {
      out.push_back('.');
      out.append(digits, 1, std::string::npos);
    }
    char ex[16];
    std::snprintf(ex, sizeof ex, "e%c%02d", e10 < 0 ? '-' : '+', std::abs(e10));
    out += ex;
  } else if (decpt <= 0) {
    out += "0.";
    out.append((size_t)-decpt, '0');
    out += digits;
  } else if (decpt >= nd) {
    out += digits;
    out.append((size_t)(decpt - nd), '0');
    out += ".0";
  } else {
    out.append(digits, 0, (size_t)decpt);
    out.push_back('.');
    out.append(digits, (size_t)decpt, std::string::npos);
  }
}

void filter_model_table(const ModelFilterArgs& a, ModelTable* out) {
  std::string text;
  {
    File in(a.table_path, "rb");
    text = in.read_all();
  }
  const std::vector<std::string> lines = stripped_lines(text);
  if (lines.empty()) throw std::invalid_argument(std::string(a.table_path) + ": no header line");
  const std::vector<std::string> head = split(lines[0], '\t');
  std::vector<size_t> keep;
  for (size_t i = 0; i < head.size(); ++i)
    if (i == 0 || i == 1 || i == 5 || i >= 10) keep.push_back(i);
  const size_t i_reads = index_of(head, "readCountSum", a.table_path), i_seqs = index_of(head, "seqCount", a.table_path);
  const std::vector<std::string> names = names_of(a.namelist), features = names_of(a.features);
  if (features.empty() || features.size() > kSvmMaxFeatures) throw std::invalid_argument("the model's selected names: 1 to 64 are taken");

  // <tmp>.csv
  std::vector<std::string> first;
  first.push_back(joined(head, keep));
  for (size_t li = 1; li < lines.size(); ++li) {
    const std::vector<std::string> c = split(lines[li], '\t');
    if (count_of(c, i_reads, li) < 10 || count_of(c, i_seqs, li) < 3) continue;
    bool has_n = false;
    for (size_t i = i_seqs; i < c.size() && !has_n; ++i) has_n = c[i] == "N";
    if (!has_n) first.push_back(joined(c, keep));
  }
  // <tmp>_refined_tmp.csv: the lines of the first file, stripped and split again as the reference reads them back
  const std::vector<std::string> h1 = split(stripped(first[0].data(), first[0].size()), ',');
  const size_t i_str = index_of(h1, "pruned_precusor_str", a.table_path);
  std::vector<std::string> second;
  second.push_back(first[0]);
  for (size_t k = 1; k < first.size(); ++k) {
    const std::vector<std::string> c = split(stripped(first[k].data(), first[k].size()), ',');
    if (i_str >= c.size()) throw std::invalid_argument("row " + std::to_string(k) + " of the first filter: no cell under pruned_precusor_str");
    if (c[i_str] != "None") second.push_back(first[k]);
  }
  // <tmp>_refined_features.csv
  std::vector<size_t> cols;
  for (size_t i = 0; i < h1.size(); ++i)
    if (std::find(names.begin(), names.end(), h1[i]) != names.end()) cols.push_back(i);
  std::vector<std::vector<std::string>> rows;   // the third file's cells, as read back from its lines
  std::vector<std::string> third;
  third.push_back(joined(h1, cols));
  for (size_t k = 1; k < second.size(); ++k) {
    third.push_back(joined(split(stripped(second[k].data(), second[k].size()), ','), cols));
    rows.push_back(split(stripped(third.back().data(), third.back().size()), ','));
  }
  const std::vector<std::string> h3 = split(stripped(third[0].data(), third[0].size()), ',');
  if (h3.size() < 3) throw std::invalid_argument(std::string(a.table_path) + ": fewer than three of the namelist's columns");
  for (size_t k = 0; k < rows.size(); ++k)
    if (rows[k].size() != h3.size())
      throw std::invalid_argument("row " + std::to_string(k) + " of the refined features: " + std::to_string(rows[k].size()) + " cells under " +
                                  std::to_string(h3.size()) + " names");

  // the feature matrix: a selected name is a column of numbers, else <column>_<value> of a column of text, else 0
  const size_t n = rows.size(), nf = features.size();
  std::vector<std::vector<double>> numeric(h3.size());   // empty = a column of text
  std::vector<uint8_t> is_numeric(h3.size(), 0);
  for (size_t ci = 3; ci < h3.size(); ++ci) {
    std::vector<double> vals(n);
    bool ok = true;
    for (size_t k = 0; k < n && ok; ++k) ok = number_of(rows[k][ci], &vals[k]);
    is_numeric[ci] = ok;
    if (ok) numeric[ci] = std::move(vals);
  }
  out->x.assign(n * nf, 0.0);
  out->n_stray = 0;
  for (size_t fi = 0; fi < nf; ++fi) {
    const std::string& f = features[fi];
    size_t hit = h3.size();
    for (size_t ci = 3; ci < h3.size() && hit == h3.size(); ++ci)
      if (h3[ci] == f) hit = ci;
    if (hit < h3.size() && is_numeric[hit]) {
      for (size_t k = 0; k < n; ++k) out->x[k * nf + fi] = numeric[hit][k];
      continue;
    }
    if (hit < h3.size() && n) ++out->n_stray;
    for (size_t ci = 3; ci < h3.size(); ++ci) {
      const std::string& c = h3[ci];
      if (is_numeric[ci] || f.size() <= c.size() || f.compare(0, c.size(), c) != 0 || f[c.size()] != '_') continue;
      const std::string value = f.substr(c.size() + 1);
      bool any = false;
      for (size_t k = 0; k < n && !any; ++k) any = rows[k][ci] == value;
      if (!any) continue;
      for (size_t k = 0; k < n; ++k) out->x[k * nf + fi] = rows[k][ci] == value ? 1.0 : 0.0;
      break;
    }
  }
  out->n_table = lines.size() - 1;
  out->n_dataset = first.size() - 1;
  out->n_refined = n;
  out->nf = (uint32_t)nf;
  out->header3 = h3[0] + "," + h3[1] + "," + h3[2];
  out->names.clear();
  for (size_t k = 0; k < n; ++k) out->names.push_back(rows[k][0] + "," + rows[k][1] + "," + rows[k][2]);

  // everything is worked out: now the files
  const std::pair<const char*, const std::vector<std::string>*> files[3] = {
      {a.dataset_path, &first}, {a.refined_tmp_path, &second}, {a.refined_path, &third}};
  for (const auto& f : files) {
    File o(f.first, "wb");
    std::string block;
    for (const std::string& ln : *f.second) {
      block += ln;
      block.push_back('\n');
      if (block.size() > (1u << 20)) {
        o.write(block);
        block.clear();
      }
    }
    o.write(block);
    o.close();
  }
}

void write_model_results(const ModelTable& t, const int8_t* pred, const double* prob, const char* detailed_path, const char* novel_path,
                         uint64_t* predicted, uint64_t* kept) {
  const uint64_t n = t.n_refined;
  for (uint64_t k = 0; k < n; ++k) {
    if (pred[k] != 1 && pred[k] != -1) throw std::invalid_argument("row " + std::to_string(k) + ": predictedValue is neither 1 nor -1");
    if (!std::isfinite(prob[2 * k]) || !std::isfinite(prob[2 * k + 1])) throw std::invalid_argument("row " + std::to_string(k) + ": a probability that is not finite");
  }
  const std::string header = "predictedValue,probability," + t.header3 + "\n";
  std::vector<std::string> line(n);
  const uint64_t run = env_count("MIRGE_AMD_MODEL_BLOCK_LINES", 4096);  // lines per worker and round (tests lower it)
  const uint64_t n_runs = (n + run - 1) / run;
  File detailed(detailed_path, "wb");
  File novel(novel_path, "wb");
  detailed.write(header);
  in_batches(n_runs, writer_threads(n_runs),
             [&](unsigned, uint64_t r) {
               for (uint64_t k = r * run; k < std::min(n, (r + 1) * run); ++k) {
                 std::string& ln = line[k];
                 ln = pred[k] == 1 ? "1," : "-1,";
                 append_repr(ln, std::max(prob[2 * k], prob[2 * k + 1]));   // model_predict.py:63: the larger of the two
                 ln.push_back(',');
                 ln += t.names[k];
                 ln.push_back('\n');
               }
             },
             [&](uint64_t first, unsigned live) {
               for (uint64_t r = first; r < first + live; ++r)
                 for (uint64_t k = r * run; k < std::min(n, (r + 1) * run); ++k) detailed.write(line[k]);
             });
  detailed.close();
  // the novel list: predicted 1 with at least 0.8, by (probability, line) descending
  std::vector<uint64_t> order;
  *predicted = 0;
  for (uint64_t k = 0; k < n; ++k) {
    if (pred[k] != 1) continue;
    ++*predicted;
    if (std::max(prob[2 * k], prob[2 * k + 1]) >= 0.8) order.push_back(k);
  }
  std::sort(order.begin(), order.end(), [&](uint64_t i, uint64_t j) {
    const double pi = std::max(prob[2 * i], prob[2 * i + 1]), pj = std::max(prob[2 * j], prob[2 * j + 1]);
    if (pi != pj) return pi > pj;
    const int c = line[i].compare(line[j]);
    return c != 0 ? c > 0 : i < j;
  });
  novel.write(header);
  for (uint64_t k : order) novel.write(line[k]);
  novel.close();
  *kept = order.size();
}

}  // namespace mrg
