// light_derive.h — derived triangle-light records: the records of an instance table made on the device from per-prim-mesh templates (csrc/light_derive.hip,
// "Emitters" in include/rt_abi.h).  The derived list walks the instances in index order and emits, for every instance whose prim mesh has a
// template, the template's rows in template order; record k of it is (instance, row) with the positions of k_light_records (csrc/light_records.hip), the row's
// texcoords, the prim mesh's material and the alias entry the host made for k.  tests/light_derive_checker.cpp restates it in plain C++.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_scene.h"

namespace rt {

struct LightExpandArgs {
  const uint32_t* prefix;             // numEmit + 1 words: first record of emitting instance e (word numEmit: the record count)
  const uint32_t* ids;                // numEmit words: the instance index of emitting instance e, ascending
  const uint32_t* meshFirstRow;       // per prim mesh: the first template row of the mesh (read for meshes with a template only)
  const rt_emitter_row* rows;         // the template rows of all meshes
  const rt_impt_samp* alias;          // numRecs alias entries, in record order
  const DevInstance* instances;       // the rows of the new table
  const rt_prim_mesh* primMeshes;
  const rt_vertex* vertices;          // the live array
  const uint32_t* indices;
  rt_trig_light* records;             // out, numRecs records: all 96 bytes
  rt_light_source* sources;           // out, numRecs (instance, triangle) pairs: the binding k_light_records reads
  uint32_t numEmit, numRecs;
};

// one thread per derived record
hipError_t launchLightExpand(hipStream_t stream, const LightExpandArgs& a);

}  // namespace rt
