// materials.h — material and texture edits without a new scene: re-derive the alpha records and the opacity micro-maps of the triangles whose material is dirty
// (csrc/materials.hip, "Editing materials and textures" in include/rt_abi.h).  A material is dirty when one of its alpha-relevant fields changed
// (pbrBaseColorFactor.w, alphaCutoff, alphaMode, pbrBaseColorTexture) or when an alpha byte of its base colour texture changed.  The rule is csrc/opacity_map.h's.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_scene.h"

namespace rt {

enum : uint32_t { MAT_NO_OWNER = 0xffffffffu };
// the counter words (cleared before the select pass)
enum : int { MAT_CNT_OWNERS = 0, MAT_CNT_SELECTED = 1, MAT_CNT_TEXELS_LO = 2, MAT_CNT_TEXELS_HI = 3, MAT_CNT_WORDS = 4 };

struct MaterialArgs {
  Tri48* tris;                        // the tree's leaf records: omm is rewritten for the selected ones
  AlphaRec* alphaByTri;               // ... and their copy of the alpha record
  Tri48* table;                       // the device builder's per-triangle table (indexed by globalId) or nullptr: its omm follows, so a later rebuild emits the new maps
  const TriRef* triRef;               // globalId -> (instance, primitive)
  const DevInstance* instances;
  const rt_prim_mesh* primMeshes;
  const rt_material* materials;       // the edited rows are in place
  const DevTexture* textures;
  AlphaRec* alphaRec;                 // indexed by Tri48::alphaIdx; the uvs stay, everything else is rewritten from the tables above
  uint4* ommPlane;                    // the four words per alphaIdx: the templates of rt_set_instances when they are in force, else scratch
  const uint32_t* dirtyBits;          // bit m: material m is dirty
  uint32_t* owner;                    // per alphaIdx: MAT_NO_OWNER before the select pass, then the leaf record that owns the rebuild
  uint32_t* owners;                   // the owners, compacted (numAlpha words)
  uint32_t* counters;                 // MAT_CNT_*
  uint32_t numRecs, numGlobal, numAlpha, numInstances, numPrimMeshes, numMaterials, numTextures, pad;
};

// one thread per leaf record: which records have a dirty material, and one owner per alpha record among them
hipError_t launchMaterialSelect(hipStream_t stream, const MaterialArgs& a);
// one wave per owner: the alpha record and the micro-map
hipError_t launchMaterialBuild(hipStream_t stream, const MaterialArgs& a, uint32_t numOwners);
// one thread per leaf record: the selected ones take their map and alpha record
hipError_t launchMaterialScatter(hipStream_t stream, const MaterialArgs& a);

}  // namespace rt
