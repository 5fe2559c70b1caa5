// stages.hip's traced kernels with per-vertex motion vectors (RT_VM; see the note at the top of stages.hip)
#define RT_SKY 1
#define RT_LAT 1
#define RT_VM 1
#include "stages.hip"
