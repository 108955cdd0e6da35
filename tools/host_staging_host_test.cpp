// csrc/host_staging.hpp with the host compiler: answers the queries that
// tests/test_host_staging_host.py writes to standard input, one per line, with
// one line each; the expected values stand in the test.  A query is a list of
// arrays in registration order, each "in|out present elem_bytes count"; the
// answer is
//   "in_words out_words total_words" then per array " ret:byte_offset:bytes"
// with ret what StagingLayout::add returned (the region, -1 for a NULL array,
// -2 when the layout is full; byte_offset and bytes are 0 for those).
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../dyros_robot_controller_amd/csrc/host_staging.hpp"

using drc_amd::StagingLayout;

static bool answer(const std::string& line, std::ostream& out) {
  std::istringstream is(line);
  std::vector<std::string> tok;
  for (std::string t; is >> t;) tok.push_back(t);
  if (tok.size() % 4 != 0) return false;
  StagingLayout lay;
  std::vector<int> ret;
  for (size_t a = 0; a < tok.size(); a += 4) {
    if (tok[a] != "in" && tok[a] != "out") return false;
    const int elem = std::stoi(tok[a + 2]);
    if (elem != 4 && elem != 8) return false;
    ret.push_back(lay.add(tok[a + 1] != "0", tok[a] == "out", std::stoll(tok[a + 3]), elem));
  }
  out << lay.in_words << ' ' << lay.out_words << ' ' << lay.total_words();
  for (int r : ret) {
    if (r >= lay.n) return false;
    out << ' ' << r << ':' << (r >= 0 ? lay.offset(r) * 8 : 0) << ':' << (r >= 0 ? lay.r[r].bytes : 0);
  }
  out << '\n';
  return true;
}

int main() {
  for (std::string line; std::getline(std::cin, line);)
    if (!answer(line, std::cout)) {
      std::cout << "BAD QUERY " << line << '\n';
      return 2;
    }
  return 0;
}
