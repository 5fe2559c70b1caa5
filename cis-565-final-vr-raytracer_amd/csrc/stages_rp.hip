// stages.hip's direct stage with settled primary visibility recorded and replayed (RT_REPLAY; see the note at the top of stages.hip)
#define RT_REPLAY 1
#include "stages.hip"
