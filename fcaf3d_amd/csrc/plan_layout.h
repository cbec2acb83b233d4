// The data format of the native coordinate phase (fc_plan_levels / fc_plan_maps): the ONE declaration of what every word of the
// cfg array, the `out` table, the device meta block, the pair-list counter block and a probe record means.  csrc/plan.hip and its
// kernel headers include it; fcaf3d_amd/plan.py reads the same text (_lib.parse_enums: plain enums, `NAME`, `NAME = integer` or
// `NAME = earlier names + integers`, // comments) — nothing else states a word number.  The kernel-map descriptors inside a map
// record are MAPW words of csrc/exec_ops.h (MAP_*, PAIR_*, MAP_ROUTE_*).
#ifndef FCAF3D_PLAN_LAYOUT_H
#define FCAF3D_PLAN_LAYOUT_H

enum {
  HDR = 16,            // out[0 .. HDR): the header (H_*)
  SETW = 8,            // then MAXSETS set records of SETW words (S_*)
  MAPR = 64,           // then the map records of MAPR words (MW_*), MAPS_FIXED + MAPS_PER_LEVEL * nl of them
  MAXSETS = 24,
  MAXLV = 8,           // pyramid levels
  MAPS_FIXED = 2,      // stem, pool
  MAPS_PER_LEVEL = 4,  // down, ds, same of a backbone level and the gsame of the generated set beside it
  METAW = 8,           // device ints per set in the meta block (META_*); behind all sets: rows per (set, scene)
  PAD = 64             // spare words behind the out table, the meta block and the counter block
};

enum {  // cfg: int64 words
  C_B,                 // scenes
  C_NL,                // pyramid levels
  C_NFEAT,
  C_VS,                // voxel size (double bits)
  C_FEATDIV,           // feature divisor (double bits)
  C_TOTAL,             // points of all scenes
  C_BACKWARD,          // backward tables wanted
  C_SORT_MIN,          // mask-sorted tables from this many rows (sparse.SORT_MIN_ROWS)
  C_PAIR_ROWS,         // pair-list convolution up to this many rows (sparse.PAIR_CONV_ROWS)
  C_PTS_THR,           // pts_threshold | -1: none
  C_TARGETS,           // head location arrays wanted
  C_COORDS_IN,         // pre-voxelised coords (device pointer) | 0: collate from the points
  C_FEATS_IN,          // their features
  C_PT_STRIDE,         // floats per point
  C_NECK,              // neck sets wanted
  C_VS_HEAD,           // the head's voxel size (double bits)
  C_PROBE,             // HIP-event brackets around every launch (group): fc_plan_probe_read
  CFGW = 24
};

enum {  // out[0 .. HDR)
  H_S,                 // sets
  H_NEED2,
  H_PRUNE,             // head level at which pts_threshold bites | -1
  H_NMAPS,
  H_STRUCT,            // every backbone voxel lies inside the generated sets
  H_NALL,              // head locations over all levels
  H_F0,                // level-0 feature rows
  H_TGT_PTS,
  H_TGT_SCENE,
  H_TGT_LEVEL,
  H_TGT_ORDER,
  H_TGT_SEG,
  H_NHEAD,
  H_BAD                // a coordinate outside the range of the hash keys
};

enum {  // a set record
  S_COORDS,
  S_N,
  S_STRIDE,
  S_KEYS,
  S_VALS,
  S_CAP,
  S_PARENT,            // generated from this set | -1
  S_ROWS               // union rows of the backbone level inside this generated set
};

enum {  // a map record
  MW_IN,               // set indices
  MW_OUT,
  MW_K,
  MW_NIN,
  MW_NOUT,
  MW_NBR,
  MW_NBRT,
  MW_SORT,             // forward table in mask order and ...
  MW_SORTI,            // ... its row order | 0: MW_SORT is the plain table
  MW_SORTT,            // the same for the transposed table
  MW_SORTTI,
  MW_PI,               // pair lists: in, out, pos, cnt (PAIR_IN .. PAIR_CNT of exec_ops.h), live tiles
  MW_PO,
  MW_POS,
  MW_CNT,
  MW_TILES,
  MW_TPI,              // the same of the transposed table
  MW_TPO,
  MW_TPOS,
  MW_TCNT,
  MW_TTILES,
  MW_FLAGS,            // MWF_* bits
  MW_DESC_F = 24,      // MAPW words: desc(conv, backward=false)
  MW_DESC_B = 44       // MAPW words: desc(conv, backward=true)
};

enum {  // MW_FLAGS
  MWF_SORT_ROWS = 1,
  MWF_USE_PAIRS = 2,
  MWF_DENSE = 4
};

enum {  // the meta block of a set
  META_ROWS = 0,
  META_BAD = 2         // range flag
};

enum {  // the pair-list counter block (device, read back into pinned host ints): CNT_MAP words per map, then CNT_TAIL words
  CNT_MAP = 64,        // [0 .. 27) pairs per offset of the map's table
  CNT_T = 32,          // [CNT_T .. CNT_T + 27) of its transposed table
  CNT_TAIL = MAXLV     // behind the maps: union hits per generated set; the host block goes on with nl * B + 1 segment starts
};

enum {  // probe kinds (plan.PROBE_KINDS names them, in this order)
  PK_TABLES,
  PK_VOXELIZE,
  PK_FLAGS,
  PK_FINALIZE,
  PK_GEN,
  PK_KMAPS,
  PK_CHILDREN,
  PK_FILL,
  PK_TRANSPOSE,
  PK_MASKS,
  PK_RADIX,
  PK_PERMUTE,
  PK_PAIRS,
  PK_GENROWS,
  PK_HEAD,
  PK_KINDS
};

#endif
