/* qa_flat_scene.h — the flattened, relocatable scene blob (plain C, POD only).
 *
 * This is the data contract of the drop-in boundary: the host side (XML loader + plugin
 * registries, qaray_amd/csrc/host) flattens qaray's pointer-based scene graph into ONE contiguous
 * blob; the HIP layer (include/qaray_hip.h: qa_scene_upload / qa_scene_attach_device_blob)
 * consumes it, RCCL broadcasts it between GPUs as raw bytes, and the CPU oracle (oracle/) reads
 * the very same bytes.  All cross references are indices or byte offsets from the blob start,
 * so the blob can be memcpy'd, mmap'd, broadcast or uploaded without fix-ups.
 *
 * What each table mirrors in the reference (paths relative to the reference repo):
 *   header camera frame  Renderer::ComputeScene            src/renderers/renderer.cpp:71-113
 *   qa_instance          Node + Transformation             src/core/node.h, src/core/transform.h:36-79
 *   qa_mesh + arrays     TriObj / TriMesh / cy::BVH        src/objects/objects.h:57-73,
 *                                                          src/mesh/TriMesh.h:41-111, src/ext/cyBVH.h:225-267
 *   qa_material          MtlBlinn_PhotonMap members        src/materials/MtlBlinn_PhotonMap.h:139-146
 *   qa_mtlset            Node::mtl -> MtlBlinn | MultiMtl  src/materials/materials.h:65-87
 *   qa_light             Ambient/Direct/Point/SpotLight    src/lights/lights.h:35-171
 *   qa_texmap/qa_texture TextureMap / TextureFile/Checker  src/core/texture.h:50-96, src/textures/texture.h
 *
 * Matrices are 3x3 column-major (GLM layout): m[3*c + r].
 */
#ifndef QA_FLAT_SCENE_H
#define QA_FLAT_SCENE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QA_FLAT_MAGIC   0x31534151u /* "QAS1" */
#define QA_FLAT_VERSION 1u
#define QA_BIGFLOAT     1.0e30f    /* src/core/setup.h:45 */
#define QA_MAX_NODE_DEPTH 8        /* deepest node nesting the traversal supports (reference scenes: 2) */

enum { QA_OBJ_NONE = 0, QA_OBJ_SPHERE = 1, QA_OBJ_PLANE = 2, QA_OBJ_MESH = 3 };
enum { QA_LIGHT_AMBIENT = 0, QA_LIGHT_DIRECT = 1, QA_LIGHT_POINT = 2, QA_LIGHT_SPOT = 3 };
enum { QA_TEX_CHECKER = 0, QA_TEX_FILE = 1 };

/* TexturedColor: colour (x map sample when texmap >= 0)           src/core/texture.h:74-96 */
typedef struct qa_texcolor {
  float   color[3];
  int32_t texmap;     /* index into texmaps, -1 = plain colour */
} qa_texcolor;

/* TextureMap = Transformation + Texture*                           src/core/texture.h:58-72 */
typedef struct qa_texmap {
  float   itm[9];
  float   pos[3];
  int32_t texture;    /* index into textures, -1 = map without texture (samples black) */
  int32_t pad[3];
} qa_texmap;

typedef struct qa_texture {
  int32_t  type;      /* QA_TEX_* */
  int32_t  width, height;
  int32_t  pad0;
  float    color1[3]; /* checker */
  float    color2[3];
  uint64_t off_texels; /* RGB8, row-major, width*height*3 bytes */
  uint64_t pad1;
} qa_texture;

/* Node in depth-first pre-order; instance 0 is the (object-less) root node. */
typedef struct qa_instance {
  float   tm[9];
  float   itm[9];
  float   pos[3];
  int32_t obj_type;    /* QA_OBJ_* */
  int32_t mesh;        /* mesh index for QA_OBJ_MESH, else -1 */
  int32_t mtlset;      /* index into mtlsets, -1 = node without material */
  int32_t parent;      /* -1 for the root */
  int32_t subtree_end; /* index one past the last descendant (pre-order) */
  int32_t depth;       /* root = 0 */
  int32_t pad;
} qa_instance;

/* What Node::GetMaterial() points at: one MtlBlinn (count 1, multi 0) or a MultiMtl. */
typedef struct qa_mtlset {
  int32_t first;  /* first entry in materials[] */
  int32_t count;
  int32_t multi;  /* 1: index by HitInfo::mtlID, white when mtlID >= count (materials.h:70-76) */
  int32_t pad;
} qa_mtlset;

typedef struct qa_material {
  qa_texcolor diffuse, specular, reflection, refraction, emission;
  float absorption[3];
  float ior;
  float kill;         /* Russian-roulette weight, 0.1                MtlBlinn_PhotonMap.cpp:50 */
  float gloss_spec;   /* specularGlossiness */
  float gloss_refl;   /* reflectionGlossiness (-1 when <= 1e-5)      MtlBlinn_PhotonMap.cpp:56-63 */
  float gloss_refr;
} qa_material;

typedef struct qa_light {
  int32_t type;       /* QA_LIGHT_* */
  float   intensity[3];
  float   position[3];
  float   direction[3];
  float   size;
  float   inner, outer; /* spot cone tangents                         lights.cpp:120-127 */
  int32_t pad[3];
} qa_light;

/* cy::BVH node, 28 bytes; nodes[0] unused, root = 1                  src/ext/cyBVH.h:225-267 */
typedef struct qa_bvh_node {
  float    box[6];    /* min xyz, max xyz */
  uint32_t data;      /* bit31 leaf; leaf: bits28-30 count-1, bits0-27 element offset; else child index */
} qa_bvh_node;
#define QA_BVH_LEAF_BIT      0x80000000u
#define QA_BVH_OFFSET_MASK   0x0FFFFFFFu
#define QA_BVH_COUNT_SHIFT   28
#define QA_BVH_COUNT_MASK    0x7u
#define QA_BVH_CHILD_MASK    0x7FFFFFFFu

/* One triangle: indices into the mesh's vertex / normal / texcoord arrays (-1 = absent). */
typedef struct qa_face {
  int32_t v[3];
  int32_t vn[3];
  int32_t vt[3];
  int32_t mtl;
} qa_face;

typedef struct qa_mesh {
  float    bmin[3], bmax[3];     /* TriMesh::ComputeBoundingBox           TriMesh.cpp:117-133 */
  uint32_t num_faces, num_vertices, num_normals, num_texcoords;
  uint32_t num_bvh_nodes;        /* including the unused slot 0 */
  uint32_t pad;
  uint64_t off_bvh_nodes;        /* qa_bvh_node[num_bvh_nodes] */
  uint64_t off_elements;         /* uint32_t[num_faces]  face ids in leaf order */
  uint64_t off_faces;            /* qa_face[num_faces] */
  uint64_t off_vertices;         /* float[3*num_vertices] */
  uint64_t off_normals;          /* float[3*num_normals] */
  uint64_t off_texcoords;        /* float[2*num_texcoords] */
} qa_mesh;

typedef struct qa_flat_header {
  uint32_t magic, version;
  uint64_t total_bytes;
  /* camera frame */
  float    screenA[3], screenU[3], screenV[3], screenX[3], screenY[3];
  float    cam_pos[3];
  float    dof;
  uint32_t width, height;
  uint32_t pad0;
  qa_texcolor background, environment;
  uint32_t num_instances, num_meshes, num_mtlsets, num_materials;
  uint32_t num_lights, num_texmaps, num_textures, pad1;
  uint64_t off_instances, off_meshes, off_mtlsets, off_materials;
  uint64_t off_lights, off_texmaps, off_textures;
  uint64_t reserved[5];
} qa_flat_header;

/* The header's camera block by name (scene edits, include/qaray_hip.h qa_scene_edit_camera; the host layer hands it out,
 * include/qaray_host.h qa_host_scene_camera).  The image size is not part of it. */
typedef struct qa_camera {
  float screenA[3], screenU[3], screenV[3], screenX[3], screenY[3];
  float cam_pos[3];
  float dof;
} qa_camera;

#define QA_BLOB_PTR(type, blob, off) ((const type *) ((const unsigned char *) (blob) + (off)))

#ifdef __cplusplus
}
#endif
#endif /* QA_FLAT_SCENE_H */
