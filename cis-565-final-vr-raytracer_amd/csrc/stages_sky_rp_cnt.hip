// stages.hip's direct stage with settled primary visibility recorded and replayed with sun & sky and the counters compiled in (RT_REPLAY; see the note at the top of stages.hip)
#define RT_SKY 1
#define RT_COUNT 1
#define RT_REPLAY 1
#include "stages.hip"
