/* libcrafter_hip.so -- the audit of env rows: an extension of the C ABI of crafter_hip.h, in a header of its own (as
 * crafter_hip_fingerprint.h: the core header's set of prototypes is pinned, an entry point a binding looks up by name is declared
 * beside it; the Python binding lists it in lib.EXTENSIONS).  C99, includes crafter_hip.h.
 *
 * A row of the world state is a dozen caller-owned device buffers (crafter_state_ptrs).  mat, objs and rec are primary; objmap
 * (where the maps stay in global memory), the five census columns per chunk and chunk_order / chunk_seen / nchunks_seen are
 * tables the step kernels keep in step with those three and then trust without looking.  crafter_audit recounts every such
 * table of every masked row from the primary state and says per env which invariant fails and where.
 *
 * With C = max_objects, nch = nchunk_x * nchunk_y, n = rec.nobj and k = rec.nchunks_seen clamped to their ranges, a LIVE record
 * a slot 1 .. n - 1 whose type != CRAFTER_T_NONE, a VALID one a live record with type <= CRAFTER_T_PLANT, x < W and y < H, the
 * chunk of a cell (x / 12) * nchunk_y + y / 12 and the LISTED chunks the ids < nch among chunk_order[0 .. k):
 *
 *   bit  name           holds when                                           detail: index, found, expected
 *   0    NOT_RESET      rec.episode != 0 (reported alone: nothing else of    -1, -1, -1
 *                       the row is read)
 *   1    REC            1 <= nobj <= C, 0 <= mt_pos <= 624, 0 <= step <      the first failing field in that order (0 nobj,
 *                       n_daylight, 0 <= nchunks_seen <= nch                 1 mt_pos, 2 step, 3 nchunks_seen), its value, the
 *                                                                            value clamped to the range
 *   2    PLAYER         slot 1 is a live CRAFTER_T_PLAYER record and no      the slot, its type (0: slot 1 is free or behind
 *                       other live record is one                             nobj), CRAFTER_T_PLAYER for slot 1 else -1
 *   3    OBJECT         every live record is valid                           the slot, the first of type / x / y out of range,
 *                                                                            its largest legal value
 *   4    CELL           no two valid records share a cell                    the cell x * H + y, the records on it, 1
 *   5    SLOTMAP        (only where objmap is state,                         the cell, objmap[cell], the lowest valid slot on it
 *                       crafter_slot_map_derived() == 0) objmap[x * H + y]   that objmap does not name; or, every valid record
 *                       == s for every valid slot s, and the non-zero        named: -1, the non-zero cells, the live records
 *                       objmap cells are as many as the live records
 *   6    MATERIAL       every mat cell is in 1 .. n_materials                the cell, its byte, -1
 *   7    SPACE          census columns 0, 1 of every chunk = the chunk's     the census word chunk * 5 + column, its value, the
 *                       grass and path cells                                 recount
 *   8    CREATURES      census columns 2, 3, 4 of every chunk = the valid    as SPACE
 *                       zombies, skeletons and cows standing in it
 *   9    CHUNKS         chunk_order[0 .. k) holds ids < nch, none twice;     the position in chunk_order, the id there (for a
 *                       chunk_seen[c] != 0 exactly for the listed chunks     listed chunk whose flag is clear: 0), -1 (1); or,
 *                                                                            the list and its flags in order: -1, the lowest
 *                                                                            unlisted chunk whose flag is set, -1
 *   10   CHUNK_MISSING  the chunk of every valid record, of any class, is    the slot, its chunk, -1
 *                       listed (engine.py:57, 79: World.add and World.move
 *                       create the chunk's key)
 *
 * Not state, and not read: records at or behind nobj, the T_NONE holes inside the prefix, crafter_obj.pad, semantic (an edit
 * leaves it stale), the status bits, mt, the world pool.  An out-of-range material counts as neither grass nor path; a record
 * that is not valid takes no part in CELL, SLOTMAP, CREATURES and CHUNK_MISSING; an id >= nch in chunk_order names no chunk.
 * The kernel indexes with nothing it has not bounded: the input is by definition untrusted.
 *
 *   flags:   int32 [num_envs]     the OR of (1 << bit) over the invariants that fail; 0: the row is consistent
 *   detail:  int32 [num_envs][4]  (bit, index, found, expected) of the LOWEST failing bit at that check's lowest offending index
 *                                 (whatever order the lanes reduce in); -1 where a value means nothing; a consistent row: four -1
 * mask: uint8 [num_envs] or NULL (all); rows with a zero byte are left untouched.  All pointers are device pointers.  Read-only:
 * it writes its two outputs only, draws nothing from the envs' RNG, sets no status bit and neither waits for nor looks at the
 * world pool (a pooled world is audited as the row it becomes).  Only enqueues work on `stream`; returns 0, or non-zero with
 * crafter_last_error: an output is NULL, or the area's tables exceed 64 KiB of LDS.  Additive under ABI revision 7. */
#ifndef CRAFTER_HIP_AUDIT_H_
#define CRAFTER_HIP_AUDIT_H_

#include "crafter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRAFTER_AUDIT_BITS 11
enum { CRAFTER_AUDIT_NOT_RESET = 1, CRAFTER_AUDIT_REC = 2, CRAFTER_AUDIT_PLAYER = 4, CRAFTER_AUDIT_OBJECT = 8, CRAFTER_AUDIT_CELL = 16,
       CRAFTER_AUDIT_SLOTMAP = 32, CRAFTER_AUDIT_MATERIAL = 64, CRAFTER_AUDIT_SPACE = 128, CRAFTER_AUDIT_CREATURES = 256,
       CRAFTER_AUDIT_CHUNKS = 512, CRAFTER_AUDIT_CHUNK_MISSING = 1024 };

int crafter_audit(crafter_handle* h, const uint8_t* mask, int32_t* flags, int32_t* detail, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CRAFTER_HIP_AUDIT_H_ */
