// parity_history_driver.cpp — a stand-alone driver of csrc/parity_history.h for tests/test_parity_history_cpu.py (built with -fsanitize=address,undefined).
//
// Reads a script from the file named on the command line, one call per line, and prints one line per call:
//   new          a freshly constructed history takes the place of the current one   -> "ok"
//   reset        the planes were freed or freshly allocated                         -> "ok"
//   invalidate   a setter, a *_reset call, a new scene or a new tree                -> "ok"
//   begin F      frame F is about to be enqueued                                    -> "read" | "fresh"
//   commit F     the pass of frame F is enqueued                                    -> "ok"
//   holds F      do the planes of F's parity hold frame F?                          -> "yes" | "no"
//   latest       parity of the last committed frame                                 -> "-1" | "0" | "1"
//   parity F     the parity frame F writes and the one it reads                     -> "0 1" | "1 0"
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include "parity_history.h"

int main(int argc, char** argv)
{
  if(argc != 2) { std::fprintf(stderr, "usage: %s script\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if(!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  rt::ParityHistory h;
  std::string line;
  while(std::getline(in, line)) {
    std::istringstream ls(line);
    std::string op;
    if(!(ls >> op) || op[0] == '#') continue;
    int f = 0;
    if((op == "begin" || op == "commit" || op == "holds" || op == "parity") && !(ls >> f)) { std::fprintf(stderr, "%s: no frame number\n", op.c_str()); return 2; }
    if(op == "new") { h = rt::ParityHistory{}; std::puts("ok"); }
    else if(op == "reset") { h.reset(); std::puts("ok"); }
    else if(op == "invalidate") { h.invalidate(); std::puts("ok"); }
    else if(op == "begin") std::puts(h.begin(f) ? "read" : "fresh");
    else if(op == "commit") { h.commit(f); std::puts("ok"); }
    else if(op == "holds") std::puts(h.holds(f) ? "yes" : "no");
    else if(op == "latest") std::printf("%d\n", h.last);
    else if(op == "parity") std::printf("%d %d\n", rt::frameParity(f), rt::otherParity(f));
    else { std::fprintf(stderr, "unknown call: %s\n", op.c_str()); return 2; }
  }
  return 0;
}
