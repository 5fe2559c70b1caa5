// reference.hip with the procedural sun & sky environment compiled in (see the note at the top of reference.hip)
#define RT_SKY 1
#include "reference.hip"
