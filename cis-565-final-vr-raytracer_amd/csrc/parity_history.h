// parity_history.h — when may a frame read the history a temporal pass keeps, and which frame's images does a parity hold?  
//
// Plain C++ with no device or library dependency, so that the rule can be tested without a GPU (tests/test_parity_history_cpu.py).
//
// SVGF, TAA and temporal upsampling each keep their history twice, by frame parity: the pass of frame f reads the planes of parity f-1 and writes those of
// parity f.  Nothing in the planes says which frame wrote them or whether it still counts; that lives HERE, in host state, one ParityHistory per pass next to
// the pass's planes in rt_ctx.  rt_render_frame calls begin() for every frame and every history, whether or not the pass runs (a frame without the pass breaks
// the chain: the next one must not read), uses the answer only when the pass runs, and calls commit() once the pass of the frame is enqueued; on every error
// return in between the history stays unreadable.
//
// SVGF under this rule.  Before the rule was shared, the SVGF flag was cleared only by frames with denoise == 0 and by frames that ran SVGF, not by every frame.
// The only other kind of frame is an A-Trous frame with denoising on, which exists only while the denoiser mode is A-Trous; every rt_set_denoiser call that
// changes the settings invalidates, and only an SVGF frame commits.  So on such a frame the flag is already false, and clearing it on every frame is the same.
// One difference remains: SVGF used to move `last` when it built its arguments, ahead of the launches, and now moves it at commit like the others.  The two
// orders differ only after an rt_render_frame call that failed in the middle of a frame, a state for which the ABI promises nothing.
#pragma once

namespace rt {

// the history parity frame `frames` writes, and the one it reads; defined for every int ((frames + 1) & 1 overflows at INT_MAX)
inline int frameParity(int frames) { return frames & 1; }
inline int otherParity(int frames) { return (frames & 1) ^ 1; }

struct ParityHistory {
  bool valid = false;             // the planes of parity `last` may be read by the next frame (consumed when a frame is enqueued)
  int last = -1;                  // parity of the last committed frame (-1: none since the planes were allocated)
  bool held[2] = {false, false};  // the planes of this parity hold the images of frame frame[parity]
  int frame[2] = {0, 0};

  // the planes were freed or freshly allocated
  void reset() { valid = false; last = -1; held[0] = held[1] = false; }
  // a setter, a *_reset call, a new scene or a new tree: the next frame starts without history (what the planes hold stays what it is)
  void invalidate() { valid = false; }
  // Frame `frames` is about to be enqueued.  Returns whether its pass may read the other parity's planes: the previous committed frame had that parity and
  // nothing invalidated since.  Whatever this frame's parity held is about to be overwritten, or is stale once the frame is out.
  bool begin(int frames)
  {
    const bool readable = valid && last == otherParity(frames);
    valid = false;
    held[frameParity(frames)] = false;
    return readable;
  }
  // the pass of frame `frames` is enqueued
  void commit(int frames)
  {
    const int p = frameParity(frames);
    valid = true; last = p; held[p] = true; frame[p] = frames;
  }
  // the planes of the frame's parity hold this very frame (rt_tonemap, rt_upscale_tonemap)
  bool holds(int frames) const { return held[frameParity(frames)] && frame[frameParity(frames)] == frames; }
};

}  // namespace rt
