// stages.hip's traced kernels with object motion vectors (RT_OM; see the note at the top of stages.hip)
#define RT_SKY 1
#define RT_LAT 1
#define RT_OM 1
#include "stages.hip"
