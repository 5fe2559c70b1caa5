// stage_select_driver.cpp — a stand-alone driver of csrc/stage_select.h for tests/test_stage_select_cpu.py (built with -fsanitize=address,undefined).
//
// Reads a script from the file named on the command line, one call per line, all arguments integers, and prints one line per call:
//   names                                                              -> the names of every StageBuild id in order, blank-separated
//   lat COUNTING TRAVERSAL STAGE W H ROWBEGIN ROWEND MAXDIRECT MAXINDIRECT -> "latency" | "throughput"
//   build SKY COUNTING LATENCY STAGE MOTION ACTION                     -> the name of the chosen build
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include "stage_select.h"

int main(int argc, char** argv)
{
  if(argc != 2) { std::fprintf(stderr, "usage: %s script\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if(!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string line;
  while(std::getline(in, line)) {
    std::istringstream ls(line);
    std::string op;
    if(!(ls >> op) || op[0] == '#') continue;
    if(op == "names") {
      for(int i = 0; i < rt::STAGE_BUILD_COUNT; i++) std::printf("%s%s", i ? " " : "", rt::stageBuildName(i));
      std::puts("");
    }
    else if(op == "lat") {
      int counting, traversal, stage, W, H, r0, r1, maxDirect, maxIndirect;
      if(!(ls >> counting >> traversal >> stage >> W >> H >> r0 >> r1 >> maxDirect >> maxIndirect)) { std::fprintf(stderr, "lat: nine integers\n"); return 2; }
      std::puts(rt::latencyBuild(counting != 0, traversal, stage, W, H, r0, r1, rt::LatencyTiles{maxDirect, maxIndirect}) ? "latency" : "throughput");
    }
    else if(op == "build") {
      int sky, counting, latency, stage, motion, action;
      if(!(ls >> sky >> counting >> latency >> stage >> motion >> action) || motion < 0 || motion > 2 || action < 0 || action > 2) {
        std::fprintf(stderr, "build: six integers, motion and action 0..2\n"); return 2;
      }
      std::puts(rt::stageBuildName(rt::stageBuild(sky != 0, counting != 0, latency != 0, stage, rt::StageMotion(motion), rt::PrimaryReplayAction(action))));
    }
    else { std::fprintf(stderr, "unknown call: %s\n", op.c_str()); return 2; }
  }
  return 0;
}
