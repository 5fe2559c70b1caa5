// stages.hip's traced kernels with object motion vectors (RT_OM; see the note at the top of stages.hip)
#define RT_OM 1
#include "stages.hip"
