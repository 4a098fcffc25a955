/*
 * gol.h -- C ABI of libgol, the MI355X-native generation-step engine.
 *
 * This is the drop-in boundary for the reference's hot path: the cell-actor
 * generation step of almendar/akka-game-of-life.  The reference has no FFI;
 * its "interface" is the Akka cell protocol.  Each entry point below names
 * the reference interface it replaces (paths relative to
 * src/main/scala/gameoflife/ of the reference).
 *
 * Conventions (DESIGN.md "Boundary"):
 *   - Plain C types only: POD structs, pointers and sizes.  No torch types.
 *   - Return 0 (GOL_OK) on success, a GOL_E* code otherwise; a per-context
 *     message is available from gol_last_error().  A JVM/ctypes shim maps a
 *     nonzero code to an exception, which is where the reference's supervisor
 *     Restart (BoardCreator.scala:42-45) would take over.
 *   - A context owns device memory on one GPU.  Host buffers belong to the
 *     caller.  A context is not re-entrant, but calls may arrive from any OS
 *     thread (actor dispatchers): every entry point re-binds its device.
 *   - There is no CPU fallback: a context can only be created on a HIP
 *     device; without one gol_create() fails with GOL_ENODEV.
 *
 * Host buffers (gol_load, gol_snapshot, checkpoints): bit-packed rows,
 * row = y, bit (x % 32) of 32-bit word (x / 32) is cell x (LSB first); words
 * per row = ceil(width / 32); bits at x >= width are zero.
 * Device layout (internal, a function of the geometry alone): the same rows,
 * except that tori whose rows hold an even number of words are kept
 * pair-interleaved (gol_device_layout) -- word 2k + j holds columns
 * 64k + 2b + j (bit b).  Two device planes (current / next) are swapped after
 * every pass.
 *
 * State hash (gol_hash, gol_step's per-generation hashes; DESIGN.md section
 * 5): a function of the cells alone -- the same board at the same epoch
 * hashes alike whatever the topology, layout, shard decomposition, pass
 * depth or environment.  Columns 64g .. 64g + 63 of row y form group g, with
 * canonical words E (bit b = cell 64g + 2b) and O (bit b = cell 64g + 2b + 1),
 * cells past the width dead; then
 *   hash = sum over (y, g) of (E A(y, 0) + O A(y, 1)) B(g)   (mod 2^64),
 *   A(y, 0) = ((t ^ (t >> 15)) << 1) | 1,  t = y * 0x9E3779B1 (mod 2^32),
 *   A(y, 1) = A(y, 0) + 0x6A09E666,  B(g) = murmur3 fmix32(g + 0x7F4A7C15) | 1.
 */
#ifndef GOL_H
#define GOL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): the state hash became a function of the cells alone (see the
 * header comment); the values of tori with an even word count are unchanged,
 * those of row-major boards (clipped, odd word counts) differ from version 1.
 * The entry points and structs are those of version 1.  gol_census,
 * gol_read_region, gol_write_region and gol_density were added without a new
 * version: additive entry points change nothing a version-2 caller relies on.
 * So were gol_set_active_rows, gol_active_stats_read and gol_active_rows, and
 * gol_step_series and gol_group_step_series (the fused population series),
 * and gol_find (the pattern search), and the batch engine with a handle type
 * of its own (gol_batch_geometry_get, gol_batch_create, gol_batch_destroy,
 * gol_batch_last_error, gol_batch_seed, gol_batch_load, gol_batch_snapshot,
 * gol_batch_step, gol_batch_hashes, gol_batch_epoch, gol_batch_set_chunk), and
 * its cycle detection (gol_cycle_step, gol_cycle_snapshot_generation,
 * gol_cycle_stats) and its pattern search (gol_find_batch_check,
 * gol_find_batch, gol_find_batch_set_cut, gol_find_batch_stats) and its
 * objects (gol_objects_batch_check, gol_objects_batch,
 * gol_objects_batch_stats) and its census (gol_census_batch_check,
 * gol_census_batch_begin, gol_census_batch_add, gol_census_batch_add_records,
 * gol_census_batch_read, gol_census_batch_stats) and its per-board rules
 * (gol_rules_batch_check, gol_rules_batch_set, gol_rules_batch_get) and its
 * soups (gol_soup_batch_check, gol_soup_batch, gol_soup_batch_rows). */
#define GOL_ABI_VERSION 2

/* Return codes. */
#define GOL_OK 0
#define GOL_EINVAL 1   /* bad argument / unsupported geometry               */
#define GOL_EHIP 2     /* HIP runtime error                                 */
#define GOL_ENOMEM 3   /* device or host allocation failed                  */
#define GOL_ECOMM 4    /* RCCL error / communicator not initialised         */
#define GOL_ESTATE 5   /* call not valid in the context's current state     */
#define GOL_ENODEV 6   /* no HIP device (no CPU fallback exists)            */

/* Topologies. */
#define GOL_TORUS 0        /* wrap in x and y (BASELINE.json configs 2-5)     */
#define GOL_REF_CLIPPED 1  /* reference geometry: (w+1)x(h+1) cells, neighbours
                              only from [0,w)x[0,h) (BoardCreator.scala:47-53,
                              package.scala:17-28)                            */

/* Life-like rules as (birth_mask, survive_mask): bit k set = the rule fires
 * at k live neighbours.  NextStateCellGathererActor.scala:42-44. */
#define GOL_RULE_LIFE_BIRTH 0x008u          /* B3/S23 (north_star)          */
#define GOL_RULE_LIFE_SURVIVE 0x00Cu
#define GOL_RULE_REF_LITERAL_BIRTH 0x000u   /* line 44 with a multiset count */
#define GOL_RULE_REF_LITERAL_SURVIVE 0x1F7u
#define GOL_RULE_REF_EFFECTIVE_BIRTH 0x000u /* line 42's Set collapse: the   */
#define GOL_RULE_REF_EFFECTIVE_SURVIVE 0x1FFu /* identity, what actually runs */

#define GOL_UNIQUE_ID_BYTES 128

typedef struct gol_ctx gol_ctx;

/* Board / shard description.  Replaces the BoardCreator constructor inputs
 * (boardSize, BoardCreator.scala:18; application.conf:29-35) plus the cell
 * placement (BoardCreator.scala:65-70): a context owns the row block
 * [row0, row0 + rows) of a width x height board. */
typedef struct gol_config {
    int64_t width;          /* cells per row (torus: multiple of 32), < 2^31  */
    int64_t height;         /* rows of the global board                       */
    int64_t row0;           /* first global row owned by this context         */
    int64_t rows;           /* rows owned (0 => height - row0)                */
    int32_t topology;       /* GOL_TORUS or GOL_REF_CLIPPED                   */
    uint32_t birth_mask;    /* 9-bit masks, see GOL_RULE_*                    */
    uint32_t survive_mask;
    int32_t device;         /* HIP device ordinal                             */
    int64_t vis_width;      /* REF_CLIPPED: visible columns (0 => width-1)    */
    int64_t vis_height;     /* REF_CLIPPED: visible rows    (0 => height-1)   */
} gol_config;

/* Create a shard context.  Replaces createAllInitialActors
 * (BoardCreator.scala:79-89) + CellActor construction (CellActor.scala:10,
 * 34: epochToState = Map(0 -> initialState)).  The board starts all dead at
 * epoch 0; fill it with gol_seed() or gol_load().
 * GOL_REF_CLIPPED boards on which some cell has no visible neighbour are
 * refused with GOL_EINVAL: the reference never completes a generation on them
 * (such a cell's gatherer has nobody to ask, so it never commits an epoch,
 * NextStateCellGathererActor.scala:26-27,39-58, and its neighbours' requests
 * for that epoch queue forever, CellActor.scala:75-76,92-94).  With the
 * default visible extents that is a board of size w = 0 or h = 0 (one cell
 * wide or tall) or w = h = 1 (2 x 2 cells). */
int gol_create(gol_ctx** out, const gol_config* cfg);

/* Free device memory and streams.  Replaces stopping the cell actors. */
void gol_destroy(gol_ctx* ctx);

/* Last error message of this context ("" if none); ctx may be NULL for the
 * process-wide last error (e.g. a failed gol_create). */
const char* gol_last_error(const gol_ctx* ctx);
const char* gol_strerror(int code);
int gol_abi_version(void);

/* Number of HIP devices visible to this process (0 on a CPU-only host). */
int gol_device_count(int* count);

/* Row-block decomposition used for sharding (DESIGN.md "Multi-GPU"): rank r
 * of n owns rows [row0, row0 + rows) of a board `height` rows tall.  Pure
 * host arithmetic.  Replaces the random placement of BoardCreator.scala:33-36. */
int gol_shard_rows(int64_t height, int rank, int nranks, int64_t* row0, int64_t* rows);

/* Device layout of a board (pure host arithmetic,
 * informational): *words_per_group = 2 when a torus row holds whole pairs of
 * 32-bit words (column 64g + 2b + j in bit b of word 2g + j), 1 (row-major:
 * column x in bit x % 32 of word x / 32) otherwise and on clipped boards.
 * Nothing at the boundary depends on it: host buffers are row-major and the
 * state hash is defined over the cells. */
int gol_device_layout(int32_t topology, int64_t width, int32_t* words_per_group);

/* Seed the shard with the counter-based splitmix64 board (Bernoulli(0.5)),
 * identical for any sharding; resets the epoch to 0.  Seeded stand-in for
 * BoardCreator.scala:23 (initialState = Random.nextBoolean() per cell). */
int gol_seed(gol_ctx* ctx, uint64_t seed);

/* Load the shard from host memory: `rows` x `host_pitch_words` packed words
 * (row 0 = global row row0).  Resets the epoch to 0.  Replaces the per-cell
 * initialState constructor argument (BoardCreator.scala:67-68). */
int gol_load(gol_ctx* ctx, const uint32_t* packed, int64_t host_pitch_words);

/* Advance `generations` generations.  Replaces one NextStep tick
 * (BoardCreator.scala:113-116) -> CurrentEpochMsg -> GetToNextEpoch ->
 * NextStateCellGathererActor gather/count/rule -> SetNewStateMsg commit
 * (CellActor.scala:63-91, NextStateCellGathererActor.scala:25-48), for every
 * cell of the shard at once.  If hashes_out is not NULL it receives, for each
 * generation, the shard's partial state hash (DESIGN.md "State hash"); the
 * global hash is the sum mod 2^64 of the shards' partials; hashes_out must
 * hold `generations` entries (gol_step_ex checks a capacity).  With a
 * communicator attached, G halo rows are exchanged over RCCL before every pass
 * of G generations.  Asynchronous when hashes_out is NULL (call gol_sync to
 * wait) -- except with active-row stepping on (gol_set_active_rows): a pass
 * that scans the board for its live rows waits for the scan, and with it for
 * every pass queued before it, so the call may return only once most of its
 * work is done. */
int gol_step(gol_ctx* ctx, uint32_t generations, uint64_t* hashes_out);

/* gol_step with the capacity of hashes_out (entries): GOL_EINVAL, and no
 * generation advanced, when hashes_out is not NULL and holds fewer than
 * `generations` entries.  The form a JVM binding calls with a direct buffer's
 * capacity. */
int gol_step_ex(gol_ctx* ctx, uint32_t generations, uint64_t* hashes_out, size_t hashes_capacity);

/* gol_step that also returns a population series, summed inside the step
 * kernels where the hash is summed: populations_out[g]
 * is the number of live stored cells of the shard's rows after generation
 * g + 1 of the call -- what gol_census would report as `population` at that
 * epoch (on GOL_REF_CLIPPED the sink row and column included) -- without a
 * second read of the plane and at the pass depths of a hashed step.
 * hashes_out[g] is what gol_step writes.  Either array may be NULL; `capacity`
 * is the entries of each array that is not.  Shards combine by sum, as the
 * hashes do (gol_comm_allreduce_u64).  With both arrays NULL the call is
 * gol_step(ctx, generations, NULL), asynchronous included; otherwise it
 * synchronises.  GOL_EINVAL, and no generation advanced, for a NULL context or
 * an array of fewer than `generations` entries; generations = 0 is GOL_OK. */
int gol_step_series(gol_ctx* ctx, uint32_t generations, uint64_t* hashes_out, uint64_t* populations_out,
                    size_t capacity);

/* Light-cone replay of a re-spawned shard, alone.  Replaces the reference's
 * re-born cell catching up from its neighbours' never-pruned histories
 * (BoardCreator.scala:138-154 re-deploys it, CellActor.scala:34,71-74,86 it
 * replays epoch by epoch from their answers).  ctx holds its rows at epoch e
 * (gol_restore of its own checkpoint); `above` holds the n = `generations`
 * rows just above row0 and `below` the n rows just below row0 + rows, as they
 * were at epoch e (global rows row0 - n .. row0 - 1 and row0 + rows ..
 * row0 + rows + n - 1, modulo the height on a torus; dead rows beyond a
 * clipped board's edge), row-major host rows `host_pitch_words` apart.  The
 * block n rows deeper on each side fixes the shard's rows for n generations,
 * so ctx advances n generations exactly as if its neighbours had been there,
 * while they stay where they are.  hashes_out (nullable, n entries) receives
 * the shard's per-generation partial hashes.  The context must not belong to
 * a group or ring yet (GOL_ESTATE). */
int gol_replay(gol_ctx* ctx, uint32_t generations, const uint32_t* above, const uint32_t* below,
               int64_t host_pitch_words, uint64_t* hashes_out);

/* Current epoch (CellActor.scala:39 myCurrentEpoch). */
int gol_epoch(const gol_ctx* ctx, uint64_t* epoch);

/* Block until all work queued on the context's streams is complete. */
int gol_sync(gol_ctx* ctx);

/* Partial state hash of the shard's current board. */
int gol_hash(gol_ctx* ctx, uint64_t* hash_out);

/* Copy the shard's current board to host: rows x host_pitch_words words.
 * Replaces the CellStateMsg stream to the LoggerActor
 * (CellActor.scala:89, LoggerActor.scala:30-46). */
int gol_snapshot(gol_ctx* ctx, uint32_t* packed_out, int64_t host_pitch_words);

/* Periodic snapshots without stalling the generation pipeline: the same copy
 * as gol_snapshot, started at the current epoch and finished in the
 * background while later gol_step calls run (LoggerActor's periodic board
 * dump, LoggerActor.scala:30-46, fed by one CellStateMsg per cell and epoch,
 * CellActor.scala:89).  The board is first copied on the device (one more
 * plane of HBM, allocated on first use), then to `packed_out` on a transfer
 * stream.  `packed_out` must stay valid and unread until gol_snapshot_wait
 * returns; page-locked memory (gol_host_alloc) keeps the call from blocking
 * on a staged copy.  One snapshot in flight per context (GOL_ESTATE). */
int gol_snapshot_async(gol_ctx* ctx, uint32_t* packed_out, int64_t host_pitch_words);

/* Wait for the snapshot started by gol_snapshot_async; *epoch_out (may be
 * NULL) receives the epoch the copy holds.  GOL_ESTATE if none is in flight. */
int gol_snapshot_wait(gol_ctx* ctx, uint64_t* epoch_out);

/* Non-blocking: *landed = 1 if the snapshot started by gol_snapshot_async
 * has reached the host buffer, 0 if it is still in flight (a JVM worker polls
 * this instead of blocking its actor thread; the fault path asks it of a lost
 * shard: a checkpoint that had not landed when the backend died never
 * existed).  GOL_ESTATE if none is in flight.  gol_snapshot_wait still ends
 * the snapshot. */
int gol_snapshot_query(gol_ctx* ctx, int* landed);

/* Page-locked host memory for snapshot / load buffers (the JVM side wraps it
 * in a direct ByteBuffer); free with gol_host_free. */
int gol_host_alloc(size_t bytes, void** out);
void gol_host_free(void* p);

/* State of one cell of the shard at the current epoch (0/1).  Replaces the
 * GetStateFromEpoch -> StateForEpoch exchange (CellActor.scala:71-77). */
int gol_get_cell(gol_ctx* ctx, int64_t x, int64_t y, int* state);

/* Census of the shard's rows, counted on the device in one pass over the
 * plane: the live cells and their bounding box in global coordinates
 * (inclusive; plain coordinate minima and maxima, not wrap-aware).  Replaces
 * reading a population off the LoggerActor's board dump
 * (LoggerActor.scala:30-46), which a host can only do after gol_snapshot has
 * shipped every row.  Every stored cell of the shard's rows counts -- on a
 * GOL_REF_CLIPPED board that includes the cells outside the visible extent.
 * A shard with no live cell reports population = 0, min_x = min_y = INT64_MAX
 * and max_x = max_y = -1, so shards combine by sum, elementwise min and
 * elementwise max.  Synchronises. */
typedef struct gol_census_result {
    uint64_t population;                 /* live cells of this shard's rows            */
    int64_t min_x, max_x, min_y, max_y;  /* bounding box of the live cells, global
                                            coordinates, inclusive                     */
} gol_census_result;
int gol_census(gol_ctx* ctx, gol_census_result* out);

/* Windows: read or change a w x h block of cells without moving the board.
 * gol_read_region replaces the CellStateMsg stream of the cells of a window
 * to the LoggerActor (CellActor.scala:89, LoggerActor.scala:30-46);
 * gol_write_region replaces the per-cell initialState a BoardCreator hands to
 * the cells it places (BoardCreator.scala:65-70) -- at any epoch, and without
 * gol_load's upload of every row.
 *
 * Window buffers use the host layout above: window row i, window column k is
 * bit k % 32 of word k / 32 of row i; rows are host_pitch_words apart,
 * host_pitch_words >= ceil(w / 32).  On write the bits at k >= w of a row's
 * last word are ignored; on read they are written as zero (words of a row
 * past ceil(w / 32) are not touched).
 *
 * The window: 1 <= w <= width, 1 <= h <= height, 0 <= x0 < width,
 * 0 <= y0 < height.  Window cell (k, i) is board cell ((x0 + k) mod width,
 * (y0 + i) mod height) of a torus.  On GOL_REF_CLIPPED the window must lie
 * inside the stored board: x0 + w <= width and y0 + h <= height.
 *
 * Null pointers, an unknown mode, a short pitch and windows out of range
 * return GOL_EINVAL with a message (gol_last_error) before any device work is
 * queued.
 *
 * Window rows whose board row is not one of the shard's rows
 * [row0, row0 + rows) are skipped: a write does not touch them, a read leaves
 * those rows of packed_out as they are.  A sharded caller therefore issues
 * the same call with the same buffer on every shard -- of an in-process
 * group, a loopback ring or an RCCL ring -- and gets the whole window; a
 * window that misses the shard altogether returns GOL_OK.
 *
 * gol_write_region combines the pattern into the window under `mode` and does
 * not change the epoch.  It is ordered on the context's compute stream after
 * every queued pass and after the device copy of a snapshot in flight; both
 * calls synchronise before they return, as gol_snapshot and gol_get_cell do.
 * Both are valid with a communicator or group attached: halo rows are
 * exchanged again at every pass.  Bits at x >= width stay zero. */
#define GOL_REGION_COPY  0   /* window := pattern           */
#define GOL_REGION_OR    1   /* window |= pattern           */
#define GOL_REGION_XOR   2   /* window ^= pattern           */
#define GOL_REGION_CLEAR 3   /* window &= ~pattern          */
int gol_read_region(gol_ctx* ctx, int64_t x0, int64_t y0, int64_t w, int64_t h,
                    uint32_t* packed_out, int64_t host_pitch_words);
int gol_write_region(gol_ctx* ctx, int64_t x0, int64_t y0, int64_t w, int64_t h,
                     const uint32_t* packed, int64_t host_pitch_words, int32_t mode);

/* Density map: the zoomed-out view of a window, counted on the device.  Each
 * entry is the number of live cells in a T x T tile, T = 1 << log2_tile,
 * 0 <= log2_tile <= 15 (a full tile holds at most 2^30 cells).  Replaces the
 * LoggerActor printing the board (LoggerActor.scala:30-46) at a scale where a
 * board can no longer be printed -- or shipped -- cell by cell: one pass over
 * the window's words on the device, and only the map crosses the bus.
 *
 * The window follows the rules of gol_read_region above (a torus wraps, a
 * GOL_REF_CLIPPED window lies inside the stored board, whose cells outside
 * the visible extent count as they do in gol_census).  Tiles are anchored at
 * the window origin, not at board coordinate 0: tile (k, i) covers window
 * columns k T .. min(w, (k + 1) T) - 1 and window rows i T ..
 * min(h, (i + 1) T) - 1, so the map has th = ceil(h / T) rows of
 * tw = ceil(w / T) counts and the last tile in each direction may be partial.
 * `pitch` is in counts, pitch >= tw.
 *
 * The call ADDS to counts[i * pitch + k] the live cells of tile (k, i) that
 * lie in the shard's rows [row0, row0 + rows); the caller zeroes the buffer
 * first.  Entries past tw of a map row are not touched, nor are map rows none
 * of whose board rows belong to the shard; a window that misses the shard
 * returns GOL_OK with the buffer unchanged.  A sharded caller therefore
 * issues the same call with the same zeroed buffer on every shard -- of an
 * in-process group, a loopback ring or an RCCL ring, whether or not shard
 * boundaries cut through tile rows -- and gets the whole map: the windows'
 * convention with a sum in place of a fill.
 *
 * A null context or buffer, log2_tile outside 0 .. 15, pitch < tw and a
 * window out of range return GOL_EINVAL with a message before any device
 * work is queued, and leave the buffer untouched.  The call is ordered on the
 * compute stream after every queued pass and after the device copy of a
 * snapshot in flight, and synchronises before it returns; it changes neither
 * the board, the epoch nor the hash, and is valid with a communicator or a
 * group attached.  The device grid it counts into belongs to the context and
 * grows on demand (GOL_ENOMEM if a map does not fit: 32 bits per tile). */
int gol_density(gol_ctx* ctx, int64_t x0, int64_t y0, int64_t w, int64_t h, int32_t log2_tile,
                uint32_t* counts, int64_t pitch);

/* Pattern search: every occurrence of a pattern on the board, found on the
 * device.  Replaces reading "what is where" off the LoggerActor's board dump
 * (LoggerActor.scala:30-46) -- how many gliders a gun has emitted, whether an
 * eater still stands at (x, y) -- which a host can only do after
 * gol_read_region has shipped the area: one pass over the rows that can hold a
 * match, and only the positions cross the bus.
 *
 * `pattern` and `care` are ph rows of packed words in the window layout above
 * (pattern column k is bit k % 32 of word k / 32, rows pattern_pitch_words
 * apart, pattern_pitch_words >= ceil(pw / 32)).  A care bit of 1: the cell must
 * equal the pattern bit; 0: don't care.  care = NULL cares for every cell of
 * the pw x ph box.  Bits at k >= pw are ignored in both.  1 <= pw <= 64,
 * 1 <= ph <= 64, pw <= width, ph <= height, at least one cared cell; a pattern
 * with no live cared cell (an empty 3 x 3 box) is legal.
 *
 * The window (x0, y0, w, h) follows the rules of gol_read_region above and is
 * a window of ANCHORS: an anchor is the board cell under the pattern's
 * top-left cell; the pattern itself may extend past the window.  Anchor (x, y)
 * matches iff for every cared cell (k, i) board cell (x + k, y + i) equals
 * pattern cell (k, i); the coordinates wrap modulo width and height on a
 * torus; on GOL_REF_CLIPPED cells beyond the stored board read dead, and the
 * stored cells outside the visible extent are cells like any other, as in
 * gol_census.
 *
 * out->count is exact.  xy_out receives out->returned = min(count,
 * max_matches) pairs (x, y) in global board coordinates, sorted by (y, x);
 * when count > max_matches they are some max_matches distinct matches, which
 * ones is unspecified.  max_matches = 0 with xy_out = NULL counts only.
 *
 * A shard examines the window's anchor rows it owns whose pattern rows
 * y .. y + ph - 1 are each one of its own rows or off the end of a clipped
 * board (a shard that owns the whole height of a torus therefore wraps).
 * Anchors whose pattern straddles a shard boundary are examined by no shard:
 * a sharded caller issues the same call on every shard, sums the counts,
 * merges the lists and completes the anchors in the last ph - 1 rows above
 * each boundary from a gol_read_region band (gameoflife.engine.ShardGroup.find
 * does).  A window that misses the shard returns GOL_OK with a zeroed result.
 * out->rows_searched is the number of anchor rows the search kernels were
 * launched over: where the rows that can hold a live cell are known
 * (gol_active_rows) and the pattern has a live cared cell, only anchor rows
 * with a pattern row inside them; results never depend on it.
 *
 * A null context, pattern or result, max_matches < 0, max_matches > 0 with a
 * null xy_out, sizes outside the limits, a short pitch, no cared cell and a
 * window out of range return GOL_EINVAL with a message before any device work
 * is queued, and leave xy_out and *out untouched.  The call is ordered on the
 * compute stream after every queued pass and after the device copy of a
 * snapshot in flight, and synchronises before it returns; it changes neither
 * the board, the epoch, the hash nor the live-row lists, and is valid with a
 * communicator, a loopback ring or a group attached.  The device buffers
 * (pattern, counters, hit list) belong to the context and grow on demand
 * (GOL_ENOMEM if they cannot: 16 bytes per match of max_matches). */
typedef struct gol_find_result {
    uint64_t count;          /* matches among the anchors this call examined            */
    uint64_t returned;       /* pairs written to xy_out: min(count, max_matches)        */
    uint64_t rows_searched;  /* anchor rows the search kernels were launched over       */
} gol_find_result;
int gol_find(gol_ctx* ctx, int64_t x0, int64_t y0, int64_t w, int64_t h,
             const uint32_t* pattern, const uint32_t* care, int64_t pattern_pitch_words,
             int32_t pw, int32_t ph,
             int64_t* xy_out, int64_t max_matches, gol_find_result* out);

/* Shard checkpoint = {header with epoch + geometry, packed board}.  Replaces
 * the reference's recovery state (initialState kept by the frontend,
 * BoardCreator.scala:23,144, plus each cell's never-pruned history,
 * CellActor.scala:34,81) used when a cell is re-deployed
 * (BoardCreator.scala:138-154). */
int gol_checkpoint_bytes(const gol_ctx* ctx, size_t* bytes);
int gol_checkpoint(gol_ctx* ctx, void* host_out, size_t bytes);

/* gol_checkpoint in the background (the periodic checkpoint of the fault
 * path overlapping the generations after it): the header is written now, the
 * rows follow as with gol_snapshot_async; finish with gol_snapshot_wait.
 * GOL_ESTATE while a snapshot or checkpoint is in flight. */
int gol_checkpoint_async(gol_ctx* ctx, void* host_out, size_t bytes);
int gol_restore(gol_ctx* ctx, const void* host_in, size_t bytes);

/* Multi-GPU: RCCL communicator over the ring of row-block shards.  Replaces
 * the cross-backend neighbour messages (GetStateFromEpoch/StateForEpoch over
 * Akka remote, application.conf:11-17).  Rank 0 calls gol_comm_unique_id and
 * distributes the bytes; every rank then calls gol_comm_init.  A context
 * with a communicator always runs the ring schedule (interior rows || halo
 * send/recv, then boundary rows); with nranks = 1 the torus ring closes on
 * itself (send/recv to self), which runs the RCCL path on a single GPU. */
int gol_comm_unique_id(uint8_t id_out[GOL_UNIQUE_ID_BYTES]);
int gol_comm_init(gol_ctx* ctx, const uint8_t id[GOL_UNIQUE_ID_BYTES], int rank, int nranks);

/* Tear down the context's communicator (ncclCommAbort: safe with a dead
 * peer); gol_comm_init may then join a new ring.  The shard keeps its board
 * and epoch.  Used when a lost backend is re-spawned and the survivors rebuild
 * the ring around it (gameoflife/elastic.py). */
int gol_comm_abort(gol_ctx* ctx);

/* Test transport: join the in-process loopback ring `key` as rank/nranks
 * instead of an RCCL communicator.  Contexts of one process -- one host
 * thread each, as one process per GPU would be -- then run exactly the halo
 * exchange gol_step issues over RCCL (the same send / receive list in the
 * same order, matched per (sender, receiver) pair in FIFO order like
 * ncclSend / ncclRecv) as device copies, and gol_comm_allreduce_u64 sums over
 * them.  This runs the multi-rank schedule with several ranks on one GPU,
 * where RCCL refuses a second rank.  gol_comm_abort leaves the ring. */
int gol_comm_init_loopback(gol_ctx* ctx, const char* key, int rank, int nranks);

/* Sum-reduce `count` uint64 values (mod 2^64) across the communicator in
 * place (the per-generation hash reduction). */
int gol_comm_allreduce_u64(gol_ctx* ctx, uint64_t* values, uint32_t count);

/* In-process shard group: several shard contexts of one board, in row order
 * and covering it without gaps, possibly on different GPUs (or several on
 * one), stepped in lockstep with halo rows pulled by device-to-device copies
 * (the same interior / boundary schedule as an RCCL ring).  This is how one
 * surviving GPU hosts a re-spawned shard next to its own (the reference
 * re-deploys a dead cell on a random surviving node, BoardCreator.scala:138-154).
 * Destroying a member leaves a hole: gol_group_step then fails with
 * GOL_ESTATE until the group is rebuilt.  gol_group_destroy unlinks the
 * shards without destroying them.  hashes_out receives the global hash. */
typedef struct gol_group gol_group;
int gol_group_create(gol_group** out, gol_ctx* const* shards, int n);
int gol_group_step(gol_group* group, uint32_t generations, uint64_t* hashes_out);
/* gol_group_step that also returns every shard's per-generation partial
 * hashes: partials_out[k * generations + g] = shard k's partial of generation
 * g (hashes_out required).  The fault path keeps them to check a re-spawned
 * shard's replayed partials against the recorded global hashes. */
int gol_group_step_partials(gol_group* group, uint32_t generations, uint64_t* hashes_out, uint64_t* partials_out);
/* gol_step_series over the group: the global hashes and the global
 * populations (the shards' sums); either array may be NULL, `capacity` as
 * there. */
int gol_group_step_series(gol_group* group, uint32_t generations, uint64_t* hashes_out, uint64_t* populations_out,
                          size_t capacity);
int gol_group_sync(gol_group* group);
const char* gol_group_last_error(const gol_group* group);
void gol_group_destroy(gol_group* group);

/* Batches of small boards: `boards` independent boards
 * of one geometry and rule, each at most 64 x 64 stored cells, stepped by one
 * launch; a board stays in registers for a whole launch, one 64-bit row per
 * lane.  Replaces running one BoardCreator (BoardCreator.scala:18-23, one
 * actor system per board) per soup: the reference's own default board (7 x 7
 * cells, stored 8 x 8; application.conf:32-33) is one eighth of a wave.  A
 * handle type of its own next to gol_ctx: a batch shares nothing with a
 * context, is not sharded, and owns its device memory on one GPU; the
 * conventions above (return codes, any OS thread, no CPU fallback) hold, with
 * gol_batch_last_error in gol_last_error's place (NULL: the process-wide last
 * error, e.g. of a failed gol_batch_create).
 *
 * Host buffers: row y of board i is one uint64_t at rows[(i - first) * height
 * + y], bit x = cell x; bits at x >= width are ignored on load and zero on
 * snapshot.  The device plane has the same layout.
 *
 * Geometry.  GOL_TORUS: 3 <= width, height <= 64, any value (a row is one
 * register and wraps with two shifts: not gol_config's multiple-of-32 rule).
 * GOL_REF_CLIPPED: width / height / vis_* mean what they mean in gol_config,
 * stored extents 1 .. 64; the boards gol_create refuses (a cell with no
 * visible neighbour) are refused alike.  1 <= boards <= 2^22; 9-bit rule
 * masks.  Anything else is GOL_EINVAL with a message.  The rule is evaluated
 * exactly as gol_step evaluates it on the same topology: every stored cell is
 * updated from its visible neighbours.
 *
 * A wave of 64 lanes holds boards_per_wave = 64 / height whole boards, lane l
 * row l % height of its board l / height; waves = ceil(boards /
 * boards_per_wave); device_bytes is what gol_batch_create allocates (the
 * plane, the plane of the generation before it that settle detection carries
 * between launches, and the settle words).  gol_batch_geometry_get validates
 * as gol_batch_create does and needs no device. */
typedef struct gol_batch gol_batch;
typedef struct gol_batch_config {
    int32_t boards;                  /* >= 1 */
    int32_t width, height;           /* stored cells per board, each <= 64 */
    int32_t topology;                /* GOL_TORUS or GOL_REF_CLIPPED */
    uint32_t birth_mask, survive_mask;
    int32_t device;
    int32_t vis_width, vis_height;   /* REF_CLIPPED: as gol_config (0 => width-1 / height-1) */
} gol_batch_config;
typedef struct gol_batch_geometry {
    int32_t boards_per_wave;
    int64_t waves;
    uint64_t device_bytes;
} gol_batch_geometry;
int gol_batch_geometry_get(const gol_batch_config* cfg, gol_batch_geometry* out);

/* Create a batch, every board dead at epoch 0 (GOL_ENODEV without a HIP
 * device, after the geometry has been validated); free it with
 * gol_batch_destroy (NULL: nothing happens). */
int gol_batch_create(gol_batch** out, const gol_batch_config* cfg);
void gol_batch_destroy(gol_batch* batch);
const char* gol_batch_last_error(const gol_batch* batch);

/* Seed every board: row y of board i is the splitmix64 output of counter
 * k = i * height + y -- z = seed + 0x9E3779B97F4A7C15 (k + 1), then
 * z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9, z = (z ^ (z >> 27))
 * 0x94D049BB133111EB, z ^= z >> 31 (mod 2^64) -- the low `width` bits of z.
 * Resets the epoch to 0. */
int gol_batch_seed(gol_batch* batch, uint64_t seed);

/* Load / read boards [first, first + count), count >= 1, in the host layout
 * above.  gol_batch_load resets the epoch to 0 (the boards it does not name
 * keep their cells).  Both synchronise. */
int gol_batch_load(gol_batch* batch, int64_t first, int64_t count, const uint64_t* rows);
int gol_batch_snapshot(gol_batch* batch, int64_t first, int64_t count, uint64_t* rows);

/* Advance every board `generations` generations; synchronises.
 * populations_out (nullable): [boards][generations] -- entry
 * [i * generations + g] is the number of live stored cells of board i after
 * generation g + 1 of the call; `capacity` is its size in entries.
 * settled_out (nullable): [boards] -- the smallest g in 2 .. generations such
 * that board i after g generations of this call equals board i after g - 2
 * (g = 2 compares with the board the call started from), 0 if there is none:
 * still lifes and period-2 ash.  Per call on purpose: it needs nothing from
 * earlier calls.  generations = 0 is GOL_OK and writes nothing.  The device
 * series buffer belongs to the handle and grows on demand (GOL_ENOMEM, and
 * nothing advanced, if it cannot).  GOL_EINVAL, nothing advanced and nothing
 * written, for a NULL handle or populations_out with capacity < boards *
 * generations. */
int gol_batch_step(gol_batch* batch, uint32_t generations, uint32_t* populations_out, size_t capacity,
                   uint32_t* settled_out);

/* State hash (the header comment's definition with row0 = 0 and the one
 * column group g = 0: what gol_hash returns for a context holding the same
 * cells) and population of boards [first, first + count).  Either array may be
 * NULL, not both.  Synchronises; changes nothing. */
int gol_batch_hashes(gol_batch* batch, int64_t first, int64_t count, uint64_t* hashes_out,
                     uint32_t* populations_out);

/* Generations every board has advanced since the last seed / load. */
int gol_batch_epoch(const gol_batch* batch, uint64_t* epoch);

/* Knob (results, settled_out included, never depend on it): a launch runs at
 * most this many generations, and the boards pass through HBM between
 * launches -- with settle detection on, the plane of the generation before
 * too -- so no single launch is long whatever a caller asks for.  0 = the
 * automatic value, 1024 (the chunk gol_step plans in). */
int gol_batch_set_chunk(gol_batch* batch, uint32_t generations_per_launch);

/* Cycle detection on a batch: gol_batch_step's
 * settled_out only knows still lifes and period-2 ash, and a caller of
 * gol_batch_step has to guess a generation count that every board then pays
 * for.  gol_cycle_step advances every board `generations` generations and
 * leaves exactly the boards and the epoch gol_batch_step(generations) leaves;
 * per board it reports the exact minimal period of the cycle the board has
 * entered and the generation of the call at which that was seen, and a board
 * whose cycle has been seen costs no more than one period of stepping per
 * launch, however many generations are asked for.  The names are not
 * gol_batch_*: the handle is the batch, the capability its own.
 *
 * Detection is Brent's algorithm on a fixed schedule, the same for every board
 * and, as settle detection, per call.  With x_g the board after g generations
 * of the call, snapshots are taken at t_k = 2^k - 1 (0, 1, 3, 7, 15, ...), and
 * for t_k < g <= t_{k+1} x_g is compared with x_{t_k}.  seen is the smallest
 * such g with x_g == x_{t_k} and period = seen - t_k; both are 0 if there is
 * none in this call.  The period is the minimal one: the first return to a
 * state on the cycle comes after exactly one period, and a snapshot taken
 * before the cycle is entered never recurs.  For a board that enters a cycle
 * of period L after M generations, seen = t_k + L for the smallest k with
 * t_k >= M and 2^k >= L: a block or a dead board (1, 1), a blinker (2, 3), a
 * glider on a 64 x 64 torus (256, 511).
 *
 * period_out / seen_out (either nullable): [boards].  generations = 0 is
 * GOL_OK and writes nothing.  Synchronises.  Launches go chunk by chunk under
 * gol_batch_set_chunk (results never depend on it); after each the call reads
 * two counters, and once every board has a period and the largest is at most
 * chunk + 1 the remainder goes as one launch.  The snapshots live in the plane
 * settle detection uses (a call is one or the other) and the per-board words
 * are allocated by the first gol_cycle_step call (GOL_ENOMEM, nothing
 * advanced, if they cannot be): gol_batch_geometry_get's device_bytes is what
 * gol_batch_create allocates, as before.  GOL_EINVAL for a NULL handle. */
int gol_cycle_step(gol_batch* batch, uint32_t generations, uint32_t* period_out, uint32_t* seen_out);

/* The schedule: the snapshot generation t_k that `generation` >= 1 of a call
 * is compared with (1 -> 0; 2, 3 -> 1; 4 .. 7 -> 3; 2^32 - 1 -> 2^31 - 1).
 * Pure, needs no device.  GOL_EINVAL for generation 0 (compared with nothing)
 * or a NULL snapshot_out. */
int gol_cycle_snapshot_generation(uint32_t generation, uint32_t* snapshot_out);

/* The last gol_cycle_step call of this batch: its launches, the boards that
 * had a period when it returned and the largest of those periods (0 before
 * the first call).  Any pointer may be NULL. */
int gol_cycle_stats(gol_batch* batch, uint64_t* launches, uint64_t* boards_cycled, uint32_t* max_period);

/* Pattern search on a batch: what the ash of a soup
 * run is -- how many blocks, blinkers, beehives and gliders each board holds,
 * which boards hold a given object, and where -- answered on the device for
 * every board at once: a list of patterns is matched against every board in
 * one launch, and only a [boards][patterns] table of counts and, if asked for,
 * the match bits cross the bus.  gol_find above works on contexts; a context
 * per board costs more than the search.  As with gol_cycle_* the names are not
 * gol_batch_*: the handle is the batch, the capability its own.
 *
 * A pattern is ph rows in the batch's host row layout: bit k of cells[i] is
 * pattern cell (k, i); a care bit of 1: the board cell must equal the pattern
 * bit, 0: don't care; care = NULL cares for every cell of the pw x ph box.
 * Bits at k >= pw are ignored in both.  1 <= pw <= width, 1 <= ph <= height,
 * at least one cared cell; a pattern with no live cared cell (an empty 3 x 3
 * box) is legal.
 *
 * The semantics are gol_find's ("Pattern search" above) with the window of
 * anchors the whole stored board: anchor (x, y) of board b matches pattern p
 * iff for every cared cell (k, i) board cell (x + k, y + i) equals pattern
 * cell (k, i); the coordinates wrap modulo width and height on GOL_TORUS; on
 * GOL_REF_CLIPPED cells beyond the stored board read dead, and the stored
 * cells outside the visible extent are cells like any other.  A context
 * holding a board's cells gives the same answer from gol_find.
 *
 * counts_out (required): [boards][npatterns] -- entry [b * npatterns + p] is
 * the exact number of matching anchors.  matches_out (nullable):
 * [npatterns][boards][height] -- bit x of entry [(p * boards + b) * height + y]
 * is set iff anchor (x, y) matches; bits at x >= width are zero.  The
 * capacities are sizes in entries.
 *
 * gol_find_batch synchronises and changes neither the boards, the epoch, the
 * hashes nor anything a later gol_batch_step or gol_cycle_step reads (both
 * are per call; the plane settle and cycle detection keep is not written).
 * The device buffers (pattern table, counts, match planes) belong to the
 * handle and grow on demand (GOL_ENOMEM, and nothing written, if they cannot);
 * gol_batch_geometry_get's device_bytes is what gol_batch_create allocates, as
 * before.  NULL arguments, npatterns outside 1 .. 256, sizes out of range, a
 * NULL cells, a pattern with no cared cell and a short capacity return
 * GOL_EINVAL with a message before any device work and leave both outputs
 * untouched.  gol_find_batch_check validates a pattern list for a geometry as
 * gol_find_batch does and needs no device (as gol_batch_geometry_get). */
typedef struct gol_batch_pattern {
    int32_t pw, ph;            /* 1 <= pw <= width, 1 <= ph <= height of the batch's boards */
    const uint64_t* cells;     /* ph rows, bit k = pattern column k */
    const uint64_t* care;      /* ph rows, or NULL: care for all pw x ph */
} gol_batch_pattern;
int gol_find_batch_check(const gol_batch_config* cfg, const gol_batch_pattern* patterns, int32_t npatterns);
int gol_find_batch(gol_batch* batch, const gol_batch_pattern* patterns, int32_t npatterns,
                   uint32_t* counts_out, size_t counts_capacity,
                   uint64_t* matches_out, size_t matches_capacity);

/* Knob (results never depend on it): the pattern list is cut into launches of
 * at most this many cared cells (a pattern that has more goes alone), so no
 * single launch is long whatever a caller asks for.  0 = the automatic value,
 * 2048 (DESIGN.md section 5h derives it). */
int gol_find_batch_set_cut(gol_batch* batch, uint32_t cared_cells_per_launch);

/* The last gol_find_batch call of this batch: its launches and the cared cells
 * of its patterns (0 before the first call).  Either pointer may be NULL. */
int gol_find_batch_stats(gol_batch* batch, uint64_t* launches, uint64_t* cared_cells);

/* The objects of a batch's boards: what a soup census
 * starts from -- every board cut into its objects, each with a canonical key
 * -- answered on the device for every board at once.  gol_find_batch counts
 * the patterns it is given; this says what else the ash holds, how many
 * distinct objects a board has and where the unfamiliar ones are.  The names
 * are gol_objects_batch*: the handle is the batch, the capability its own.
 *
 * Objects.  Two live stored cells of a board are linked iff their Chebyshev
 * distance is at most `reach` (1 or 2): cyclic in both directions on
 * GOL_TORUS, plain on GOL_REF_CLIPPED, where the stored cells outside the
 * visible extent are cells like any other (as for gol_find_batch).  An object
 * is a connected component of the link graph.  reach = 1 is 8-connectivity,
 * reach = 2 groups islands that can influence a common cell.  What
 * gol_find_batch finds of a pattern inside `reach` rings of cared dead cells
 * is an object with the pattern's record; the search also wants the rings'
 * corners dead, which are further than `reach` from an object that does not
 * fill the corners of its box.
 *
 * Order.  A board's objects are numbered by their first cell in row-major
 * order of plain stored coordinates (smallest y, then smallest x).
 *
 * Bounding box.  Clipped: the plain minimum and maximum.  Torus, per axis: the
 * object's occupied columns (rows) leave at most one cyclic run of at least
 * `reach` empty columns -- two would disconnect it.  With such a run, x is the
 * column after it and w is width minus its length; without, the object goes
 * round the axis: x = 0, w = width.  So w == width on a torus always means
 * "goes round".
 *
 * Hash.  The state hash (gol_hash, gol_batch_hashes) of the object translated
 * so that its box corner is cell (0, 0), cyclically on a torus and by 0 on an
 * axis it goes round: what gol_batch_hashes returns for a board that holds
 * only the object at its corner, whatever the board's size.
 *
 * counts_out: [count] -- entry [b - first] is the exact number of objects of
 * board b (at most 1024: two live cells of one 2 x 2 tile are always linked).
 * objects_out: [count][max_objects] -- entry [(b - first) * max_objects + j] is
 * object j of board b for j < min(its count, max_objects); the records past
 * that are all-zero (a real object has population >= 1).  The capacities are
 * sizes in entries.  first and count select boards as in gol_batch_hashes.
 *
 * gol_objects_batch synchronises and changes neither the boards, the epoch,
 * the hashes nor anything a later gol_batch_step, gol_cycle_step or
 * gol_find_batch reads (the plane settle and cycle detection keep is not
 * written).  The device buffers (counts, records) belong to the handle and
 * grow on demand (GOL_ENOMEM, and nothing written, if they cannot);
 * gol_batch_geometry_get's device_bytes is what gol_batch_create allocates, as
 * before.  NULL arguments, reach outside {1, 2}, max_objects outside
 * 1 .. 1024, a board range outside the batch and a short capacity return
 * GOL_EINVAL with a message before any device work and leave both outputs
 * untouched.  gol_objects_batch_check validates the same arguments for a
 * geometry and needs no device (as gol_batch_geometry_get). */
typedef struct gol_batch_object {      /* 16 bytes */
    uint64_t hash;                     /* translation-invariant key, above */
    uint8_t  x, y;                     /* bounding-box corner, stored coordinates */
    uint8_t  w, h;                     /* bounding-box extents, 1 .. 64 */
    uint16_t population;               /* live cells of the object, 1 .. 4096 */
    uint16_t reserved;                 /* 0 */
} gol_batch_object;
int gol_objects_batch_check(const gol_batch_config* cfg, int64_t first, int64_t count,
                            int32_t reach, int32_t max_objects);
int gol_objects_batch(gol_batch* batch, int64_t first, int64_t count, int32_t reach, int32_t max_objects,
                      uint32_t* counts_out, size_t counts_capacity,
                      gol_batch_object* objects_out, size_t objects_capacity);

/* The last gol_objects_batch call of this batch: its launches, the objects it
 * found in all (the sum of its counts) and the boards whose count exceeded
 * max_objects (0 before the first call).  Any pointer may be NULL. */
int gol_objects_batch_stats(gol_batch* batch, uint64_t* launches, uint64_t* objects, uint64_t* boards_truncated);

/* The census of a batch's objects: how many of each
 * object, over all boards and over as many calls (reseeds) as the caller
 * likes, and one place to look each of them up -- kept in a hash table on the
 * device that belongs to the handle, filled from the records
 * gol_objects_batch's kernel leaves in device memory, and read back once as a
 * short sorted list.  The names are gol_census_batch*.
 *
 * Key.  (hash, w, h, population) of a gol_batch_object record.  Every value of
 * hash is a legal key, 0 and all-ones included.
 *
 * gol_census_batch_begin allocates, or clears, a table for max_keys distinct
 * keys, 1 .. GOL_CENSUS_BATCH_MAX_KEYS: its capacity is the power of two
 * >= 2 * max_keys, in slots of 32 bytes.  It resets the call ordinal and the
 * statistics and may be called again at any time.  The table belongs to the
 * handle, is freed by gol_batch_destroy and is not part of
 * gol_batch_geometry_get's device_bytes, which stays what gol_batch_create
 * allocates.  GOL_ENOMEM: nothing is changed -- a census begun before goes on.
 *
 * gol_census_batch_add runs the objects launch of gol_objects_batch (reach,
 * max_objects as there) over all boards at their current state into the
 * handle's objects buffers, tallies every real record -- j < min(count,
 * max_objects) of each board -- and synchronises.  It changes nothing that
 * gol_batch_step, gol_cycle_step, gol_find_batch or gol_objects_batch reads or
 * returns: boards, epoch, hashes and the plane settle and cycle detection
 * keep.  *call_out (may be NULL) is this call's ordinal: 0, 1, ... since
 * begin; the caller keeps ordinal -> seed.  Ordinals stop at 2^24 - 1: the
 * next add is refused.
 *
 * gol_census_batch_add_records tallies n caller-supplied records (n <= 2^22;
 * those with population 0 are skipped) as if they were board `board`'s
 * (< 2^22), and takes an ordinal like add: how censuses of other handles,
 * processes or GPUs are merged (an entry as count records would be too many:
 * the merge is of what objects calls returned).
 *
 * Accounting, exact and always:
 *     seen = tallied + truncated + overflowed,   sum of entry.count = tallied.
 * seen: for add the sum of the boards' exact counts, for add_records the
 * records with a population; truncated: the sum over boards of
 * max(count - max_objects, 0); overflowed: below.
 *
 * Overflow.  A key is stored only within min(capacity, 256) linear probes of
 * its home slot, so a lookup that does not find it there knows it is absent,
 * and no probe loop is longer.  An object whose key finds neither itself nor
 * a free slot there is counted in overflowed and nowhere else.  With distinct
 * <= max_keys (load <= 0.5) no overflow is expected; beyond that, which keys
 * are kept is unspecified, and overflowed > 0 tells the caller to begin again
 * with more room.
 *
 * Exemplar.  first_call, first_board, first_y, first_x: the minimum of (call,
 * board, y, x) over the key's occurrences, x and y the box corner.
 * Deterministic.
 *
 * gol_census_batch_read compacts the occupied slots on the device, copies
 * them out and sorts them on the host by (count descending, hash, w, h,
 * population): the output is identical from run to run.  *n_out is the number
 * of distinct keys; capacity (in entries) below it returns GOL_EINVAL with
 * *n_out set and entries_out untouched.  It does not clear the census.
 *
 * gol_census_batch_stats: the add / add_records calls since begin, and seen,
 * tallied, truncated, overflowed, distinct as above (zeros before begin).  Any
 * pointer may be NULL.
 *
 * NULL handles, add / add_records / read before begin, reach outside {1, 2},
 * max_objects outside 1 .. 1024, max_keys outside 1 .. 2^20 and n above 2^22
 * return GOL_EINVAL with a message before any device work.
 * gol_census_batch_check validates reach, max_objects and max_keys for a
 * geometry and needs no device. */
#define GOL_CENSUS_BATCH_MAX_KEYS (1 << 20)
typedef struct gol_census_entry {      /* 32 bytes */
    uint64_t hash;                     /* gol_batch_object.hash */
    uint8_t  w, h;                     /* its box extents */
    uint16_t population;
    uint32_t first_call;               /* ordinal of the add call of the earliest occurrence */
    uint64_t count;                    /* objects with this key since begin */
    uint32_t first_board;              /* ... its board, */
    uint8_t  first_x, first_y;         /* ... its box corner */
    uint16_t reserved;                 /* 0 */
} gol_census_entry;
int gol_census_batch_check(const gol_batch_config* cfg, int32_t reach, int32_t max_objects, int64_t max_keys);
int gol_census_batch_begin(gol_batch* batch, int64_t max_keys);
int gol_census_batch_add(gol_batch* batch, int32_t reach, int32_t max_objects, uint32_t* call_out);
int gol_census_batch_add_records(gol_batch* batch, const gol_batch_object* records, size_t n, uint32_t board,
                                 uint32_t* call_out);
int gol_census_batch_read(gol_batch* batch, gol_census_entry* entries_out, size_t capacity, size_t* n_out);
int gol_census_batch_stats(gol_batch* batch, uint64_t* calls, uint64_t* seen, uint64_t* tallied,
                           uint64_t* truncated, uint64_t* overflowed, uint64_t* distinct);

/* Per-board rules: a rule sweep in one launch -- one
 * soup, or one soup per rule, under as many rules as the batch has boards.  A
 * batch is created with one rule, its configuration's; gol_rules_batch_set
 * gives boards [first, first + count) rules of their own, and from then on
 * gol_batch_step and gol_cycle_step advance board i under rule i: bit for bit
 * what board i of a batch created with rule i and holding the same cells
 * does -- the boards after any number of generations, populations_out,
 * settled_out, period_out, seen_out and the epoch, whatever
 * gol_batch_set_chunk says.  Everything that looks at cells only
 * (gol_batch_hashes, gol_find_batch, gol_objects_batch, gol_census_batch_*)
 * works on such a batch unchanged.  As with gol_cycle_* the names are not
 * gol_batch_*: the handle is the batch, the capability its own.
 *
 * A rule is one uint32_t word per board: the birth mask in bits 0..8 and the
 * survive mask in bits 16..24, GOL_BATCH_RULE(birth, survive); a word with any
 * other bit set is refused.
 *
 * gol_rules_batch_set: boards first .. first + count - 1 take rules[0 ..
 * count - 1]; the boards never named keep the configuration's rule.  It
 * changes neither the boards nor the epoch.  rules == NULL with first == 0 and
 * count == boards returns the batch to its configuration's rule and to the
 * kernels a batch without per-board rules runs (rules == NULL with any other
 * range is refused).  GOL_EINVAL, with nothing changed and the index of the
 * offending word in the message, for a bad word; GOL_EINVAL, with nothing
 * changed, for a range outside the batch or a NULL handle.  The first call
 * allocates the device's [boards] words (GOL_ENOMEM, and nothing changed, if
 * it cannot); gol_batch_destroy frees them, and gol_batch_geometry_get's
 * device_bytes stays what gol_batch_create allocates, as for the cycle words
 * and the census.  Synchronises.
 *
 * gol_rules_batch_get: the rules in force for boards [first, first + count),
 * the configuration's word where none was set.  Needs no device work.
 *
 * gol_rules_batch_check validates first, count and rules for a geometry as
 * gol_rules_batch_set does, and needs no device. */
#define GOL_BATCH_RULE(birth, survive) ((uint32_t)(((uint32_t)(birth) & 0x1FFu) | (((uint32_t)(survive) & 0x1FFu) << 16)))
int gol_rules_batch_check(const gol_batch_config* cfg, int64_t first, int64_t count, const uint32_t* rules);
int gol_rules_batch_set(gol_batch* batch, int64_t first, int64_t count, const uint32_t* rules);
int gol_rules_batch_get(gol_batch* batch, int64_t first, int64_t count, uint32_t* rules_out);

/* Soups: the boards a soup search starts from,
 * generated on the device -- a random window of any density in an otherwise
 * dead board, under one of nine symmetries, soup number n a pure function of
 * (seed, n) so that a census entry's first_call and first_board lead back to
 * the soup that produced it.  gol_batch_seed keeps its own definition (every
 * stored cell a fair coin).  The names are gol_soup_batch*: the handle is the
 * batch, the capability its own.
 *
 * Raw bits.  mix(seed, c) is gol_batch_seed's function of a counter:
 * z = seed + 0x9E3779B97F4A7C15 (c + 1), z = (z ^ (z >> 30))
 * 0xBF58476D1CE4E5B9, z = (z ^ (z >> 27)) 0x94D049BB133111EB, z ^= z >> 31
 * (mod 2^64).  For soup number s, window row v and bit plane j in 0..7,
 * Z[j] = mix(seed, (s * 64 + v) * 8 + j) (mod 2^64); window column u has the
 * 8-bit value t(u) = sum over j of (bit u of Z[j]) << j, and raw(u, v) is
 * t(u) < density: a cell lives with probability density / 256.
 *
 * Symmetry.  On window coordinates X is (u, v) -> (w - 1 - u, v), Y is
 * (u, v) -> (u, h - 1 - v), T is (u, v) -> (v, u) and R is (u, v) ->
 * (h - 1 - v, u); T and R need w == h.  The groups: C1 {e}; C2 {e, XY};
 * C4 {e, R, R^2, R^3}; D2_X {e, X}; D2_Y {e, Y}; D2_DIAG {e, T};
 * D4_PLUS {e, X, Y, XY}; D4_DIAG {e, T, XY, T XY}; D8 all eight.  Window cell
 * (u, v) is raw(u*, v*), (u*, v*) the member of the orbit of (u, v) under the
 * group with the smallest (v', u') in lexicographic order.  The parity of w
 * and h decides whether an axis runs through cells or between them.  Stored
 * cell (x + u, y + v) of the board takes that value and every other stored
 * cell is dead, on both topologies: on a clipped board the stored cells
 * outside the visible extent are cells like any other.
 *
 * gol_soup_batch: boards first .. first + count - 1 become soups index0 + b,
 * b the board's number in the batch (mod 2^64), so giving a part of a batch
 * its soups again reproduces the boards it had; the other boards keep their
 * cells.  It resets the epoch to 0 as gol_batch_load does, and keeps the
 * per-board rules.  One launch; synchronises.
 *
 * gol_soup_batch_rows writes the same boards to host memory in the host
 * layout ([count][height]; capacity in entries) and needs neither a device
 * nor a handle: a census exemplar's soup comes back from
 * (seed, index0 + first_board) in any process.
 *
 * Refused with GOL_EINVAL and a message, before any device work and with
 * nothing written: a NULL argument, w < 1 or h < 1, a window not inside the
 * stored board (x, y >= 0, x + w <= width, y + h <= height; no wrap), density
 * outside 1 .. 255, an unknown symmetry, w != h with C4, D2_DIAG, D4_DIAG or
 * D8, boards [first, first + count) outside the batch, and for
 * gol_soup_batch_rows a capacity below count * height.  gol_soup_batch_check
 * validates the same arguments for a geometry and needs no device.  The
 * device's 64 domain words belong to the handle (GOL_ENOMEM, and nothing
 * changed, if they cannot be had) and are not part of
 * gol_batch_geometry_get's device_bytes. */
#define GOL_SOUP_C1 0
#define GOL_SOUP_C2 1
#define GOL_SOUP_C4 2
#define GOL_SOUP_D2_X 3
#define GOL_SOUP_D2_Y 4
#define GOL_SOUP_D2_DIAG 5
#define GOL_SOUP_D4_PLUS 6
#define GOL_SOUP_D4_DIAG 7
#define GOL_SOUP_D8 8
typedef struct gol_soup_spec {
    uint64_t seed;
    uint64_t index0;     /* board b holds soup number index0 + b (mod 2^64) */
    int32_t  x, y, w, h; /* the window, in stored cells; the rest of the board is dead */
    int32_t  density;    /* 1 .. 255: a cell lives with probability density / 256 */
    int32_t  symmetry;   /* GOL_SOUP_C1 .. GOL_SOUP_D8 */
} gol_soup_spec;         /* 40 bytes */
int gol_soup_batch_check(const gol_batch_config* cfg, const gol_soup_spec* spec, int64_t first, int64_t count);
int gol_soup_batch(gol_batch* batch, const gol_soup_spec* spec, int64_t first, int64_t count);
int gol_soup_batch_rows(const gol_batch_config* cfg, const gol_soup_spec* spec, int64_t first, int64_t count,
                        uint64_t* rows_out, size_t capacity);

/* Kernel timing: when enabled, the dominant step-kernel launch of every pass
 * (the whole shard, or a sharded shard's interior rows) is bracketed by HIP
 * events on the stream it runs on.  gol_profile_read returns, since the last
 * reset, the summed duration (ms), the number of launches and the number of
 * generations those launches advanced (a pass may fuse several). */
int gol_profile_enable(gol_ctx* ctx, int enable);
int gol_profile_read(gol_ctx* ctx, double* total_ms, uint64_t* launches, uint64_t* generations);
int gol_profile_reset(gol_ctx* ctx);
/* Clock (GHz) the GPU held during the profiled launches since the last
 * reset, time-weighted: each launch's workgroups read their XCD's core-clock
 * and 100 MHz reference counters at start and end (0 if none recorded). */
int gol_profile_clock(gol_ctx* ctx, double* ghz);

/* Per-rank breakdown of the profiled passes of a sharded context (the cost
 * of the cross-backend exchange the reference carries as GetStateFromEpoch /
 * StateForEpoch messages, CellActor.scala:71-77,
 * NextStateCellGathererActor.scala:32-36).  Since the last
 * gol_profile_reset, with profiling enabled:
 *   kernel_ms / launches / generations: as gol_profile_read (the dominant
 *       launch: the whole shard, or a sharded shard's interior rows);
 *   exchange_ms / exchanges: the halo exchange of each sharded pass, timed by
 *       HIP events on the comm stream around the RCCL group (or loopback
 *       copies): from the moment the plane is final to the moment every send
 *       and receive of the pass has completed -- waiting for a late peer
 *       included;
 *   boundary_ms / boundary_launches: the boundary-row launches on the edge
 *       stream;
 *   halo_bytes_sent / halo_bytes_received: bytes posted to / expected from
 *       the ring's send and receive operations (counted whether or not
 *       profiling is enabled);
 *   clock_ghz: as gol_profile_clock;
 *   exchange_exposed_ms / pass_tail_ms: per pass, how long after the end of
 *       its interior launch the exchange (resp. the boundary launch) ended,
 *       0 if before, summed: the part of the exchange the interior did not
 *       hide (so at most the exchange itself, where the interior ended before
 *       the exchange began), and the pass's whole critical path beyond the
 *       interior.  The two sums cover ring passes: a shard of an in-process
 *       group adds 0 to both. */
typedef struct gol_profile_stats {
    double kernel_ms;
    uint64_t launches;
    uint64_t generations;
    double exchange_ms;
    uint64_t exchanges;
    double boundary_ms;
    uint64_t boundary_launches;
    uint64_t halo_bytes_sent;
    uint64_t halo_bytes_received;
    double clock_ghz;
    double exchange_exposed_ms;  /* sum over passes of how long the exchange ended after the interior launch (>= 0) */
    double pass_tail_ms;         /* ... and the boundary launch: the pass's critical path beyond the interior */
} gol_profile_stats;
int gol_profile_stats_read(gol_ctx* ctx, gol_profile_stats* out);

/* The runtime stack this process's libgol is bound to: the HIP runtime and
 * RCCL versions it calls and the files the dynamic linker resolved them to
 * (dladdr of a symbol of each), plus libgol's own path.  Host-only: needs no
 * device.  A JVM host and the Python tools report the same fields, so a
 * multi-rank run states which library stack it exercised. */
typedef struct gol_runtime_info {
    int32_t abi_version;
    int32_t hip_runtime_version;  /* hipRuntimeGetVersion (0 if it failed)  */
    int32_t hip_driver_version;   /* hipDriverGetVersion  (0 if it failed)  */
    int32_t rccl_version;         /* ncclGetVersion, e.g. 22707 = 2.27.7    */
    char hip_library[512];        /* path of the libamdhip64 in use         */
    char rccl_library[512];       /* path of the librccl in use             */
    char gol_library[512];        /* path of this libgol                    */
} gol_runtime_info;
int gol_runtime_info_get(gol_runtime_info* out);

/* Tuning knobs (results never depend on them); 0 selects the automatic
 * choice, which is also the default of a new context:
 *   band_rows       rows of output streamed by one wave;
 *   gens_per_pass   generations fused per HBM pass (temporal blocking, 1..12;
 *                   automatic: the pass planner, see gol_pass_plan);
 *   words_per_lane  32-bit words each lane owns per row (1, 2 or 4; must
 *                   divide the words of a row).
 * GOL_EINVAL for words_per_lane = 4 together with gens_per_pass > 7 on any
 * board but the B3/S23 torus: those kernel instances (generic rule masks,
 * clipped visibility) would spill registers to scratch and are not built
 * (the planner caps planned passes of such a tuning at 7). */
int gol_set_tuning(gol_ctx* ctx, int32_t band_rows, int32_t gens_per_pass, int32_t words_per_lane);

/* Active-row stepping, a knob like the tuning: results
 * never depend on it -- boards, epochs, hashes, census, snapshots and
 * checkpoints are bit-identical with it on or off.  enable: 0 off (the
 * default of a new context), 1 on; GOL_EINVAL otherwise.  With it on, a pass
 * steps only the row runs that can hold a live cell (the rows written through
 * gol_write_region or found by a device scan, grown by the pass depth) and
 * clears what the destination plane held elsewhere, so a small pattern on a
 * huge board advances in time proportional to the pattern.  Rows only, and
 * only on a context stepped whole: while a communicator, a loopback ring or a
 * shard group is attached, and for rules with birth on 0 neighbours, the mode
 * is accepted and every pass steps the whole plane as before.  A board that
 * is live all over falls back to whole-plane passes and is scanned again
 * after ever longer waits (4, 16, 64, then every 256 passes).  May be switched
 * at any epoch. */
int gol_set_active_rows(gol_ctx* ctx, int32_t enable);

typedef struct gol_active_stats {
    uint64_t passes;        /* passes run since the last reset, mode on            */
    uint64_t sparse_passes; /* ... of them stepped as row runs                      */
    uint64_t rows_stepped;  /* output rows launched, summed over passes             */
    uint64_t rows_cleared;  /* rows zeroed in the destination plane                 */
    uint64_t scans;         /* device scans for live rows ...                       */
    uint64_t rows_scanned;  /* ... and the rows they read                           */
} gol_active_stats;
/* The counters of this context; reset != 0 zeroes them after reading. */
int gol_active_stats_read(gol_ctx* ctx, gol_active_stats* out, int32_t reset);

/* Diagnostic: the runs [lo, hi) (global rows) outside which the current plane
 * is known dead, as at most max_runs pairs in lo_hi_pairs (may be NULL when
 * max_runs is 0) and their number in *count; *count = -1 when nothing is known
 * (after gol_seed, gol_load, a sharded pass ...).  Kept in either mode. */
int gol_active_rows(gol_ctx* ctx, int64_t* lo_hi_pairs, int32_t max_runs, int32_t* count);

/* Diagnostic: the pass depths (generations fused per HBM pass) gol_step would
 * use to advance `generations` generations (at most 1024: gol_step plans per
 * chunk of 1024) with or without per-generation hashes, in launch order.
 * Writes at most `max` depths to `depths` and their number to `count`. */
int gol_pass_plan(gol_ctx* ctx, uint32_t generations, int32_t with_hashes, int32_t* depths, int32_t max,
                  int32_t* count);

/* Diagnostic: resident 64-lane waves per CU of the step kernel a pass of
 * `gens_per_pass` generations would launch with the context's current
 * tuning (occupancy API), and the strip width in words (a whole row for the
 * whole-row waves of a 4096-column B3/S23 torus at 10-generation passes). */
int gol_occupancy(gol_ctx* ctx, int32_t gens_per_pass, int32_t* waves_per_cu, int32_t* strip_words);

/* Diagnostic: runs a one-wave kernel exercising the cross-lane primitives the
 * step kernel relies on (DPP wave shifts, v_alignbit, scalar loads) and
 * writes 256 words to report (layout: gol_kernels.hip selftest_kernel). */
int gol_selftest(int device, uint32_t* report);

/* Diagnostics of the HIP status discipline.  A failing
 * HIP call leaves its status pending on the calling thread (hipGetLastError);
 * libgol takes every status it reports or logs off the thread, launches its
 * kernels with calls that return their own status, and absorbs what RCCL's
 * own HIP calls leave behind right after each RCCL call.  So after any libgol
 * entry point the thread has no pending HIP status that libgol produced.
 *   gol_diag_take_hip_error: the calling thread's pending HIP status (0: none),
 *                            taken off the thread (hipGetLastError).
 *   gol_diag_absorbed:       how many statuses RCCL calls left behind, and the
 *                            last one's description (`last` may be NULL). */
int gol_diag_take_hip_error(int* code);
int gol_diag_absorbed(uint64_t* count, char* last, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* GOL_H */
