// primary_replay_driver.cpp — a stand-alone driver of csrc/primary_replay.h for tests/test_primary_replay_cpu.py (built with -fsanitize=address,undefined).
//
// Reads a script from the file named on the command line, one call per line, and prints one line per call:
//   rest N                         at-rest launches ahead of a recording for the calls that follow (the header clamps to >= 2)
//   cam NAME                       the current camera becomes NAME (created on first use: every name a different viewInverse)
//   flip NAME BIT                  flip bit BIT (0..511) of NAME's projInverse words
//   history NAME                   change NAME's projView, lastView, lastProjView, lastPosition and nbLights: none of them is part of a view
//   size W H                       the image size of the launches that follow
//   launch [band] [ineligible]     one direct launch with the current camera and size     -> "normal" | "record" | "replay"
//   invalidate                     an invalidating call (rt_update_instances, rt_resize, ...) -> "dropped"
//   state                          -> "state N atRest M"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "primary_replay.h"

int main(int argc, char** argv)
{
  if(argc != 2) { std::fprintf(stderr, "usage: %s script\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if(!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  rt::PrimaryReplayState s;
  std::map<std::string, rt_scene_camera> cams;
  std::string cur;
  int rest = 2, W = 70, H = 50;
  auto get = [&](const std::string& name) -> rt_scene_camera& {
    auto it = cams.find(name);
    if(it == cams.end()) {
      rt_scene_camera c{};
      for(int i = 0; i < 16; i++) { c.viewInverse.m[i] = float(cams.size() + 1) * 0.25f + float(i); c.projInverse.m[i] = 1.0f / float(i + 1); }
      it = cams.emplace(name, c).first;
    }
    return it->second;
  };
  std::string line;
  while(std::getline(in, line)) {
    std::istringstream ls(line);
    std::string op;
    if(!(ls >> op) || op[0] == '#') continue;
    if(op == "rest") { ls >> rest; std::puts("ok"); }
    else if(op == "cam") { ls >> cur; (void)get(cur); std::puts("ok"); }
    else if(op == "flip") {
      std::string n; int bit = 0; ls >> n >> bit;
      if(bit < 0 || bit >= 512) { std::fprintf(stderr, "flip: bit out of range\n"); return 2; }
      uint32_t w; rt_scene_camera& c = get(n);
      std::memcpy(&w, &c.projInverse.m[bit / 32], 4); w ^= 1u << (bit % 32); std::memcpy(&c.projInverse.m[bit / 32], &w, 4);
      std::puts("ok");
    }
    else if(op == "history") {
      std::string n; ls >> n; rt_scene_camera& c = get(n);
      for(int i = 0; i < 16; i++) { c.projView.m[i] += 1.0f; c.lastView.m[i] -= 2.0f; c.lastProjView.m[i] += 0.5f; }
      c.lastPosition.x += 1.0f; c.lastPosition.y -= 1.0f; c.lastPosition.z += 3.0f; c.nbLights += 1;
      std::puts("ok");
    }
    else if(op == "size") { ls >> W >> H; std::puts("ok"); }
    else if(op == "launch") {
      rt::PrimaryReplayLaunch l{};
      l.view = rt::primaryReplayViewOf(get(cur), W, H);
      l.fullFrame = true; l.eligible = true;
      std::string flag;
      while(ls >> flag) { if(flag == "band") l.fullFrame = false; else if(flag == "ineligible") l.eligible = false; else { std::fprintf(stderr, "launch: unknown flag\n"); return 2; } }
      const rt::PrimaryReplayAction a = rt::primaryReplayStep(s, l, rest);
      std::puts(a == rt::PRIMARY_REPLAY_RECORD ? "record" : (a == rt::PRIMARY_REPLAY_REPLAY ? "replay" : "normal"));
    }
    else if(op == "invalidate") { rt::primaryReplayInvalidate(s); std::puts("dropped"); }
    else if(op == "state") std::printf("state %d atRest %d\n", s.state, s.atRest);
    else { std::fprintf(stderr, "unknown call: %s\n", op.c_str()); return 2; }
  }
  return 0;
}
