/*
 * chgpu.h — C ABI of the MI355X-native block-processing hot path (filter -> aggregate -> hash join).
 *
 * This is the drop-in boundary.  The reference (filimonov/ClickHouse) has no C ABI for this path; its extension
 * points are C++ virtual interfaces.  Every entry point below names the reference interface it stands in for
 * (file:line relative to the reference checkout); INTEGRATION.md shows the C++ shim a maintainer adds on the
 * reference side (GpuFilterTransform : ISimpleTransform, GpuAggregator, GpuHashJoin : IJoin) that calls these.
 *
 * Conventions
 *   - plain C, opaque handles, no torch/HIP types in signatures (a hipStream_t travels as void*);
 *   - every call returns an int status: 0 = OK, negative = error mapped from the reference's error names;
 *     chgpu_last_error() gives the message of the calling thread's last failure; nothing throws across the ABI;
 *   - the caller owns host buffers; the library owns device buffers behind handles;
 *   - a chgpu_ctx binds one device + one HIP stream; N host threads drive N contexts concurrently (the
 *     threading contract of IProcessor::work(), src/Processors/IProcessor.h:176-193); one ctx is single-threaded, but MAY be used
 *     from different threads one after another: every entry point makes the context's device current for the duration of
 *     the call and restores the caller's (a fresh pipeline thread starts on device 0);
 *   - CHGPU_ERR_NOT_IMPLEMENTED means "fall back to the CPU path" (mirror of isCompilable() gating,
 *     src/AggregateFunctions/AggregateFunctionSum.h:590-604).
 */
#ifndef CHGPU_H
#define CHGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHGPU_ABI_VERSION 1

/* ---- status codes (names follow src/Common/ErrorCodes.cpp) ---- */
enum
{
    CHGPU_OK = 0,
    CHGPU_ERR_SIZES_MISMATCH = -1,  /* SIZES_OF_COLUMNS_DOESNT_MATCH (ColumnVector.cpp:685-686) */
    CHGPU_ERR_NOT_IMPLEMENTED = -2, /* NOT_IMPLEMENTED: caller falls back to CPU */
    CHGPU_ERR_OOM = -3,             /* CANNOT_ALLOCATE_MEMORY */
    CHGPU_ERR_LOGICAL = -4,         /* LOGICAL_ERROR */
    CHGPU_ERR_BAD_ARGUMENTS = -5,   /* BAD_ARGUMENTS */
    CHGPU_ERR_DEVICE = -6,          /* a HIP runtime call failed */
    CHGPU_ERR_TOO_MANY_ROWS = -7    /* TOO_MANY_ROWS (HashJoin.cpp:563-564: block >= 2^32 rows; Aggregator::checkLimits,
                                       Aggregator.cpp:1816-1830: max_rows_to_group_by exceeded under group_by_overflow_mode THROW) */
};

/* ---- column element types (the TypeIndex subset of the hot path, src/Core/TypeId.h) ----
   Every entry point takes every type unless it says otherwise; arithmetic (chgpu_arith) and the fused expression kernel
   (chgpu_expr_filter_sum) are limited to the integers among the first six and answer CHGPU_ERR_NOT_IMPLEMENTED for Float64 /
   UInt16 / Int16 / Int8 / Float32; keys (GROUP BY, join, sharding, packed) are integers. */
enum
{
    CHGPU_I64 = 0,
    CHGPU_U32 = 1,
    CHGPU_U64 = 2,
    CHGPU_F64 = 3,
    CHGPU_U8 = 4,
    CHGPU_I32 = 5,
    CHGPU_U16 = 6, /* also Date (days since epoch) */
    CHGPU_I16 = 7,
    CHGPU_I8 = 8,
    CHGPU_F32 = 9  /* sums and averages accumulate in Float64 (SumSimple: NearestFieldType<Float32>) */
};

/* ---- comparison functions (src/Functions/FunctionsComparison.h: equals..greaterOrEquals) ---- */
enum { CHGPU_EQ = 0, CHGPU_NE = 1, CHGPU_LT = 2, CHGPU_GT = 3, CHGPU_LE = 4, CHGPU_GE = 5 };

/* ---- aggregate functions with POD states the device can hold (src/AggregateFunctions/) ---- */
enum { CHGPU_AGG_COUNT = 0, CHGPU_AGG_SUM = 1, CHGPU_AGG_AVG = 2,
       /* min / max over a numeric argument, result in the argument's type (AggregateFunctionsMinMax.cpp, SingleValueDataFixed: SingleValueData.cpp:
          219-262); with a GROUP BY key (hash table states) or without (one reduction per block).  The 8-byte state word is an order key: merge /
          export / import as for the sums, but never through the wire serialisation of chgpu_agg_serialize_states. */
       CHGPU_AGG_MIN = 3, CHGPU_AGG_MAX = 4,
       /* any(x): the value of the group's FIRST row in the order the blocks were added (AggregateFunctionAny.cpp: setIfFirst; merges keep the
          state that already has a value -- changeFirstTime).  Two 8-byte state words {claim, value}: the claim names the earliest row, so the
          result does not depend on the order the hardware serves the rows in. */
       CHGPU_AGG_ANY = 5,
       /* argMin(arg, val) / argMax(arg, val) over numeric columns (AggregateFunctionArgMinMax.h; SingleValueData.cpp setIfSmaller /
          setIfGreater): the `arg` of the FIRST row, in the order rows were added over all blocks, whose `val` is the group's minimum /
          maximum -- a later row replaces the state only when its val is strictly smaller / greater.  The result has arg's type and arg's
          bits untouched (Float32 as any() treats it).
          TWO ARGUMENTS: arg_types (chgpu_agg_create) and every arg_cols array (add_block, add_block_filtered, execute_on_block) are indexed
          by ARGUMENT SLOT.  These kinds own two consecutive slots, arg then val; every other kind owns one, so with none of these kinds
          present slot j is aggregate j.  arg and val may each be any of the ten column types.
          THREE 8-byte public state words per aggregate, in table order {val word, has, arg bits}: val word is val's order key (complemented for
          argMin, as min / max export theirs), has is 0 for "no value" and non-zero otherwise -- an import reads any non-zero value as "has
          a value, older than every row to come" -- and arg bits are as any() exports its value.  A merge keeps the destination's {val, arg}
          unless the source's val is strictly greater (argMax) / smaller (argMin); equal vals keep the destination's, and a row that
          later only equals a merged-in extremum loses to it.  A state without a value (an overflow row nobody reached, no key and no
          rows) loses every merge and finalizes to arg's default, 0.
          Zeros: -0.0 and +0.0 in val are equal to the reference's comparison, so the val order key folds the zero's sign away: such rows
          tie and the first wins (min / max keep their own key: they return the value).
          NaN in val takes the place it has in the min / max order key (above +inf / below -inf by its sign), where the reference's answer
          depends on which row came first -- the same documented deviation as for min / max.
          Never through chgpu_agg_serialize_states / deserialize_states. */
       CHGPU_AGG_ARG_MIN = 6, CHGPU_AGG_ARG_MAX = 7 };

/* ---- JoinKind / JoinStrictness subset (src/Core/Joins.h) ---- */
enum { CHGPU_JOIN_INNER = 0, CHGPU_JOIN_LEFT = 1, CHGPU_JOIN_RIGHT = 2, CHGPU_JOIN_FULL = 3 }; /* RIGHT / FULL: strictness ALL only */
enum { CHGPU_STRICT_ANY = 0, CHGPU_STRICT_ALL = 1, CHGPU_STRICT_SEMI = 2, CHGPU_STRICT_ANTI = 3 };

typedef struct chgpu_ctx chgpu_ctx;
typedef struct chgpu_col chgpu_col;
typedef struct chgpu_agg chgpu_agg;
typedef struct chgpu_join chgpu_join;

/* ================================================================================================
 * context
 * ============================================================================================== */
int chgpu_abi_version(void);
const char * chgpu_last_error(void);
/* hip_stream: an existing hipStream_t to launch on (e.g. the host framework's stream), or NULL for a private one */
int chgpu_ctx_create(int device_id, void * hip_stream, chgpu_ctx ** out);
/* Columns, aggregations, joins and communicators made on a context keep it alive: destroying a context that still has children only
   marks it, and the last child to be freed tears it down (no use-after-free whatever order a garbage collector picks). */
int chgpu_ctx_destroy(chgpu_ctx * ctx);
int chgpu_ctx_synchronize(chgpu_ctx * ctx);
/* give the context's cached device memory (column pool + scratch arena) back to the driver; synchronizes */
int chgpu_ctx_trim(chgpu_ctx * ctx);
/* Developer options: plan-level A/B switches and launch geometry (names: tools/README.md; e.g. "tune_join_no_radix", "tune_gb_tile").  No
   operator reads the environment: an option is set here, per context, or with ctx == NULL as the process-wide default.  Unknown names ->
   CHGPU_ERR_BAD_ARGUMENTS.  Results never depend on an option (only the plan taken does). */
int chgpu_ctx_set_option(chgpu_ctx * ctx, const char * name, int64_t value);
/* ProfileEvents-style counters of this context (src/Common/ProfileEvents.cpp:1034-1035, 245-247):
   [0] FilterTransformPassedRows [1] FilterTransformPassedBytes [2] JoinBuildTableRowCount
   [3] JoinProbeTableRowCount [4] JoinResultRowCount [5] AggregatedRows [6] kernel launches [7] table rehashes */
#define CHGPU_N_COUNTERS 8
int chgpu_ctx_counters(chgpu_ctx * ctx, uint64_t out[CHGPU_N_COUNTERS]);
/* HIP-event stopwatch on the context's stream (IProcessor::elapsed_ns analogue, IProcessor.h:359-364) */
int chgpu_timer_start(chgpu_ctx * ctx);
int chgpu_timer_stop_ms(chgpu_ctx * ctx, double * elapsed_ms); /* synchronizes on the stop event */

/* ================================================================================================
 * a1/a2 columns: PaddedPODArray<T> pinned into HBM (src/Common/PODArray.h:51-57; IColumn::Filter =
 * PaddedPODArray<UInt8>, src/Columns/FilterDescription.h:14).  Device buffers are over-allocated by 64 B on both
 * sides like the reference's pad so kernels may over-read a vector lane.
 * ============================================================================================== */
int chgpu_col_upload(chgpu_ctx * ctx, int type, const void * host_ptr, uint64_t rows, chgpu_col ** out);
int chgpu_col_alloc(chgpu_ctx * ctx, int type, uint64_t rows, chgpu_col ** out);
/* Pinned, double-buffered staging (the StripeBuilder of the host shim): chgpu_host_alloc gives page-locked host memory; an upload from it
   is queued on the context's COPY stream and returns at once -- the copy overlaps whatever kernels are already queued on the
   context's stream, and everything the caller launches on that stream afterwards sees the column (an event orders them).  The host
   buffer may be refilled once chgpu_upload_wait(ticket) has returned. */
int chgpu_host_alloc(size_t bytes, void ** out);
int chgpu_host_free(void * p);
int chgpu_col_upload_async(chgpu_ctx * ctx, int type, const void * pinned_host_ptr, uint64_t rows, chgpu_col ** out, uint64_t * ticket_out);
int chgpu_upload_wait(chgpu_ctx * ctx, uint64_t ticket);
/* non-owning view of caller-managed HBM (columns already resident on the device) */
int chgpu_col_wrap(chgpu_ctx * ctx, int type, void * device_ptr, uint64_t rows, chgpu_col ** out);
/* IColumn::cut(start, length) as a non-owning view (src/Columns/IColumn.h:118-121) */
int chgpu_col_slice(chgpu_ctx * ctx, const chgpu_col * col, uint64_t start, uint64_t rows, chgpu_col ** out);
/* concatenation of n columns of one type (the way right-side Blocks are glued into one payload column: ColumnVector::insertRangeFrom,
   src/Columns/ColumnVector.cpp:511-526) */
int chgpu_col_concat(chgpu_ctx * ctx, uint32_t n, const chgpu_col * const * cols, chgpu_col ** out);
int chgpu_col_download(chgpu_ctx * ctx, const chgpu_col * col, void * host_ptr, uint64_t rows);
/* every column of a (result) Block to host memory with ONE wait: host_ptrs[c] receives all rows of cols[c] */
int chgpu_col_download_many(chgpu_ctx * ctx, uint32_t n, const chgpu_col * const * cols, void * const * host_ptrs);
uint64_t chgpu_col_rows(const chgpu_col * col);
int chgpu_col_type(const chgpu_col * col);
void * chgpu_col_device_ptr(const chgpu_col * col);
int chgpu_col_free(chgpu_col * col);

/* ================================================================================================
 * §8(f) rank 3 — the feed side: compressed frames decoded in HBM.  A MergeTree column file / compressed Native stream is a
 * sequence of frames: 16-byte checksum, method byte, compressed size (incl. the 9-byte header), decompressed size, payload
 * (src/Compression/CompressedReadBufferBase.cpp:175-222, CompressionInfo.h:10-51).  The host walks the frame headers and verifies the
 * checksums (chgpu_compressed_walk_frames / chgpu_read_compressed_column below), uploads the compressed bytes once and names the
 * frames; every frame is decoded by one wavefront straight into the output buffer (LZ4 block format as in
 * LZ4_decompress_faster.cpp:470-684; method 0x02 NONE copies).  CODEC(Delta, LZ4) -- a Multiple frame (0x91,
 * CompressionCodecMultiple.cpp:68-130) whose methods are {0x92, 0x82} -- is two stages: the host names the inner LZ4 stage's payload
 * and output size (stage_sizes) and sets post_methods[f] = 0x92; the Delta stage (CompressionCodecDelta.cpp:84-175: running sums) checks
 * its own header on the device.  post_methods / stage_sizes may be NULL.  Other methods -> CHGPU_ERR_NOT_IMPLEMENTED; a malformed frame ->
 * CHGPU_ERR_BAD_ARGUMENTS (CANNOT_DECOMPRESS), never a fault.  chgpu_col_from_bytes turns a byte range of the result into a typed
 * column (SerializationNumber::deserializeBinaryBulk: plain little-endian arrays).
 * ============================================================================================== */
/* The frame walk itself, with the reference's integrity checks (CompressedReadBufferBase.cpp:49-127,130-222): every frame's checksum --
   CityHash128 (cityhash 1.0.2) over header + payload, stored in front of it as {low64, high64} -- is verified unless verify_checksums == 0
   (the reference's disable_checksum), compressed / decompressed sizes above 1 GiB (DBMS_MAX_COMPRESSED_SIZE) are refused, a Multiple{Delta,
   LZ4} frame is split into its stages.  `file` is host memory.  Fills up to `capacity` entries of the arrays chgpu_decompress_frames takes
   and returns the number of frames (call with capacity 0 to validate and count).  A mismatch answers CHGPU_ERR_BAD_ARGUMENTS with the
   reference's message ("Checksum doesn't match: corrupted data." ...). */
int chgpu_compressed_walk_frames(const uint8_t * file, uint64_t size, int verify_checksums, uint32_t capacity, uint32_t * n_frames, uint64_t * payload_offsets,
                                 uint32_t * payload_sizes, uint32_t * decompressed_sizes, uint8_t * methods, uint8_t * post_methods, uint32_t * stage_sizes);
/* CompressedReadBuffer + SerializationNumber::deserializeBinaryBulk in one call: a MergeTree `<column>.bin` / compressed Native stream of a
   numeric column in host memory -> a typed column in HBM (walk + verify on the host, the compressed bytes cross PCIe, decode on the device) */
int chgpu_read_compressed_column(chgpu_ctx * ctx, const uint8_t * file, uint64_t size, int type, int verify_checksums, chgpu_col ** out);
/* CityHash_v1_0_2::CityHash128 (the checksum of a frame a writer has to put in front of it): out = {low64, high64} */
int chgpu_city_hash128(const void * data, uint64_t size, uint64_t out_low_high[2]);
/* Native format (src/Formats/NativeReader.cpp:113-260): the header walk of ONE block in host memory.  [BlockInfo when server_revision > 0:
   (field, value)* 0 with field 1 = is_overflows, 2 = bucket_num (src/Core/BlockInfo.cpp:38-62)] columns, rows (VarUInt), then per column
   name, type name (strings), [a custom-serialization flag byte from revision 54454 on] and the values.  The walk describes where every
   column's parts lie; the caller moves them to HBM:
     numbers (kind NUMERIC): rows x sizeof(T) little-endian bytes at data_offset (chgpu_col_upload / chgpu_col_upload_async);
     FixedString(N) (FIXED_STRING): rows x N bytes at data_offset, a UInt8 column for chgpu_fixed_string_word;
     String (STRING): (VarUInt length, bytes) per value in [data_offset, +data_bytes), chars_bytes of them value bytes -> chgpu_native_read_strings;
     Nullable(T) of these: is_nullable = 1 and the null map's rows bytes at null_map_offset, in front of the nested values
       (SerializationNullable; chgpu_filter_description_nullable / NullableKeyAggregator take the map);
     LowCardinality(String) and LowCardinality(Nullable(String)) (LC_STRING): SerializationLowCardinality.cpp:84-164,:560-700 -- keys version
       (must be 1), index type + flags (a global dictionary is refused, additional keys are required: the reference's messages), lc_num_keys
       keys serialized as Strings in [lc_keys_offset, +lc_keys_bytes) (chgpu_native_read_strings; is_nullable: key 0 stands for NULL), then
       rows indexes of `type` (UInt8/16/32/64) at data_offset, each checked against lc_num_keys ("Index for LowCardinality is out of
       range", ColumnLowCardinality.cpp:240-252).  Indexes + dictionary are a ColumnLowCardinality for chgpu_lc_remap / GROUP BY / joins.
   Any other type answers CHGPU_ERR_NOT_IMPLEMENTED.  *bytes_consumed = where the next block starts.
   Parity pin: tests/golden/native_lc_blocks.json = the bytes and messages of tests/queries/0_stateless/02010_lc_native.{python,reference}. */
enum
{
    CHGPU_NATIVE_NUMERIC = 0,
    CHGPU_NATIVE_STRING = 1,
    CHGPU_NATIVE_FIXED_STRING = 2,
    CHGPU_NATIVE_LC_STRING = 3
};
typedef struct chgpu_native_column
{
    char name[64];
    char type_name[64];
    int32_t type;         /* CHGPU_* element type: the values' (NUMERIC), UInt8 (STRING / FIXED_STRING), the indexes' (LC_STRING) */
    int32_t kind;         /* CHGPU_NATIVE_* */
    uint32_t fixed_n;     /* FixedString(N) */
    int32_t is_nullable;
    uint64_t data_offset; /* byte offset of the column's values inside `data` */
    uint64_t data_bytes;
    uint64_t null_map_offset;
    uint64_t chars_bytes; /* STRING: sum of the value lengths */
    uint64_t lc_num_keys, lc_keys_offset, lc_keys_bytes, lc_keys_chars_bytes;
} chgpu_native_column;
int chgpu_native_walk_block(const uint8_t * data, uint64_t size, uint64_t server_revision, uint32_t capacity, chgpu_native_column * columns, uint32_t * n_columns,
                            uint64_t * n_rows, int32_t * bucket_num, int * is_overflows, uint64_t * bytes_consumed);
/* `rows` serialized String values (SerializationString::deserializeBinaryBulk) in host memory -> a ColumnString in HBM */
int chgpu_native_read_strings(chgpu_ctx * ctx, const uint8_t * serialized, uint64_t bytes, uint64_t rows, chgpu_col ** offsets_u64, chgpu_col ** chars_u8);
int chgpu_decompress_frames(chgpu_ctx * ctx, const chgpu_col * compressed_u8, uint32_t n_frames, const uint64_t * payload_offsets,
                            const uint32_t * payload_sizes, const uint32_t * decompressed_sizes, const uint8_t * methods,
                            const uint8_t * post_methods, const uint32_t * stage_sizes, chgpu_col ** out_u8);
int chgpu_col_from_bytes(chgpu_ctx * ctx, const chgpu_col * bytes_u8, uint64_t byte_offset, int type, uint64_t rows, chgpu_col ** out);

/* ================================================================================================
 * a3 comparison  —  IFunction::executeImpl for less/greater/equals... with a constant right argument:
 * NumComparisonImpl<A,B,Op>::vectorConstant (src/Functions/FunctionsComparison.h:204-245), semantics
 * accurate::lessOp/equalsOp (src/Core/AccurateComparison.h:20-130).  mask[i] = Op(col[i], scalar) ? 1 : 0.
 * Supported: integer column x integer scalar of any signedness, F64 x F64, integer column x F64 scalar and F64 column x
 * integer scalar -- all compared mathematically (a constant no value of the column type can equal compares accordingly;
 * NaN is unequal to everything and unordered).
 * ============================================================================================== */
int chgpu_cmp_const(chgpu_ctx * ctx, const chgpu_col * col, int op, int scalar_type, const void * scalar,
                    chgpu_col ** mask_u8);

/* ================================================================================================
 * a4/a5 filter  —  IColumn::filter(const Filter &, ssize_t result_size_hint) (src/Columns/IColumn.h:313-314;
 * ColumnVector<T>::filter, src/Columns/ColumnVector.cpp:682-724).  Order-preserving; any non-zero mask byte keeps
 * the row; size mismatch -> CHGPU_ERR_SIZES_MISMATCH.  result_size_hint: <0 reserve rows, >0 reserve hint, 0 exact.
 * ============================================================================================== */
int chgpu_count_bytes_in_filter(chgpu_ctx * ctx, const chgpu_col * mask_u8, uint64_t * count); /* ColumnsCommon.cpp:31-58 */
int chgpu_filter(chgpu_ctx * ctx, const chgpu_col * col, const chgpu_col * mask_u8, int64_t result_size_hint,
                 chgpu_col ** out, uint64_t * out_rows);
/* The same for every column of a Block at once -- FilterTransform::doTransform's loop over the chunk's columns
   (src/Processors/Transforms/FilterTransform.cpp:238-252) and joinBlock's filtering of the left columns
   (src/Interpreters/HashJoin/HashJoinMethodsImpl.h:122-123): the mask is counted and scanned once, one host synchronisation
   for the whole Block.  outs[k] receives column k filtered; all have out_rows rows. */
int chgpu_filter_columns(chgpu_ctx * ctx, uint32_t n_cols, const chgpu_col * const * cols, const chgpu_col * filter_u8,
                         int64_t result_size_hint, chgpu_col ** outs, uint64_t * out_rows);
/* a6 FilterDescription for Nullable(UInt8): res = data && !null (src/Columns/FilterDescription.cpp:86-92) */
int chgpu_filter_description_nullable(chgpu_ctx * ctx, const chgpu_col * data_u8, const chgpu_col * null_u8, chgpu_col ** out);

/* ================================================================================================
 * a8/a9 aggregate functions without key  —  IAggregateFunction::addBatchSinglePlace
 * (src/AggregateFunctions/IAggregateFunction.h:254-260): AggregateFunctionSumData::addMany /
 * addManyConditional (AggregateFunctionSum.h:62-236).  state8 is the 8-byte host-side state (Int64 for signed,
 * UInt64 for unsigned, Float64 for floats: SumSimple, AggregateFunctionSum.cpp:19-28); the batch sum is ADDED to it.
 * ============================================================================================== */
int chgpu_sum_add_many(chgpu_ctx * ctx, const chgpu_col * col, uint64_t row_begin, uint64_t row_end, void * state8);
int chgpu_sum_add_many_conditional(chgpu_ctx * ctx, const chgpu_col * col, const chgpu_col * cond_u8,
                                   uint64_t row_begin, uint64_t row_end, void * state8);

/* Fused a3+a5+a8/a9 for `SELECT sum(val), count() WHERE pred <op> scalar` (FilterTransform::doTransform,
 * src/Processors/Transforms/FilterTransform.cpp:136-256 -> Aggregator::executeWithoutKeyImpl,
 * src/Interpreters/Aggregator.cpp:1276-1321): one pass over HBM, no mask, no filtered column.
 * val may equal pred.  sum_out: 8 bytes typed like SumSimple(val type). */
int chgpu_filter_sum(chgpu_ctx * ctx, const chgpu_col * pred, int op, int scalar_type, const void * scalar,
                     const chgpu_col * val, void * sum_out, uint64_t * count_out);
/* same, no host synchronisation: result_u64x2 is a 2-row CHGPU_U64 device column receiving {sum bits, count} */
int chgpu_filter_sum_async(chgpu_ctx * ctx, const chgpu_col * pred, int op, int scalar_type, const void * scalar,
                           const chgpu_col * val, chgpu_col * result_u64x2);

/* ================================================================================================
 * SURVEY §8(f) rank 1 — pieces of the expression DAG an SSB Q1.1-style query needs, and their fusion.
 * `and`: FunctionAnd over UInt8 columns (AndImpl::apply = a & b, src/Functions/FunctionsLogical.h:82-96).
 * multiply / plus / minus: FunctionBinaryArithmetic (src/Functions/multiply.cpp:10-28) with NumberTraits result types
 * (src/DataTypes/NumberTraits.h:73-87): integer operands of <= 8 bytes give a 64-bit result, unsigned only for
 * multiply/plus of two unsigned operands; wrap-around arithmetic.  Float operands -> CHGPU_ERR_NOT_IMPLEMENTED.
 * ============================================================================================== */
enum { CHGPU_VAL_COL = 0, CHGPU_VAL_MUL = 1, CHGPU_VAL_PLUS = 2, CHGPU_VAL_MINUS = 3 };
int chgpu_and(chgpu_ctx * ctx, const chgpu_col * a_u8, const chgpu_col * b_u8, chgpu_col ** out_u8);
int chgpu_arith(chgpu_ctx * ctx, int value_op, const chgpu_col * a, const chgpu_col * b, chgpu_col ** out);
/* Fused `SELECT sum(<value>), count() WHERE p_0 AND p_1 ...` in ONE pass over HBM (ExpressionActions::execute +
 * FilterTransform + AggregatingTransform without key).  cols[n_cols] are the distinct columns touched (<= 4; Int64, UInt64,
 * UInt32, Int32 or UInt8 in any mix of widths, each 16-byte aligned, all of one row count; Float64 / Float32 / 2-byte / Int8
 * columns, a fifth column, a ninth predicate or a misaligned view -> CHGPU_ERR_NOT_IMPLEMENTED); predicate k is
 * `cols[pred_col[k]] pred_op[k] constant` (constant = 8 raw bytes in pred_scalar_bits[k], typed pred_scalar_type[k];
 * <= 8 predicates, and-ed); value = cols[val_a] (CHGPU_VAL_COL) or cols[val_a] <op> cols[val_b].
 * sum_out: 8 bytes, Int64 or UInt64 per the result type rules above (*result_type_out tells which). */
int chgpu_expr_filter_sum(chgpu_ctx * ctx, uint32_t n_cols, const chgpu_col * const * cols, uint32_t n_preds,
                          const uint32_t * pred_col, const int * pred_op, const int * pred_scalar_type,
                          const uint64_t * pred_scalar_bits, int value_op, uint32_t val_a, uint32_t val_b,
                          int * result_type_out, void * sum_out, uint64_t * count_out);

/* ------------------------------------------------------------------------------------------------
 * The general form: an expression DAG compiled at run time into ONE kernel (hiprtc, gfx950) -- ExpressionActions::execute
 * (src/Interpreters/ExpressionActions.cpp:595-747) without materialised intermediates; the counterpart of the reference's
 * compile_expressions JIT (src/Interpreters/JIT/CHJIT.cpp, compileFunction.cpp).  A program is an array of nodes in
 * topological order (operands precede their users); result types follow src/DataTypes/NumberTraits.h, comparisons
 * src/Core/AccurateComparison.h (mixed-sign and integer-vs-float operands compared mathematically; NaN as there), logical
 * functions see static_cast<bool>(x) (FunctionsLogical.cpp:81,424), date functions take a Date (CHGPU_U16 day number).
 * Type combinations the reference answers with a type this path does not carry (128-bit, Float -> integer casts, if() over
 * UInt64 and a signed type) give CHGPU_ERR_NOT_IMPLEMENTED at compile time: the caller keeps its CPU actions.
 * ---------------------------------------------------------------------------------------------- */
enum { CHGPU_EX_INPUT = 0, CHGPU_EX_CONST = 1, CHGPU_EX_FUNC = 2 };
enum
{
    CHGPU_FN_EQUALS = 0, CHGPU_FN_NOT_EQUALS = 1, CHGPU_FN_LESS = 2, CHGPU_FN_GREATER = 3, CHGPU_FN_LESS_OR_EQUALS = 4,
    CHGPU_FN_GREATER_OR_EQUALS = 5,                                   /* = CHGPU_EQ .. CHGPU_GE; result UInt8 */
    CHGPU_FN_PLUS = 10, CHGPU_FN_MINUS = 11, CHGPU_FN_MULTIPLY = 12,  /* ResultOfAdditionMultiplication / ResultOfSubtraction */
    CHGPU_FN_DIVIDE = 13,                                             /* Float64 (ResultOfFloatingPointDivision) */
    CHGPU_FN_NEGATE = 14,                                             /* ResultOfNegate */
    CHGPU_FN_INT_DIV = 15, CHGPU_FN_MODULO = 16,                      /* integers, constant divisor that cannot raise ILLEGAL_DIVISION */
    CHGPU_FN_AND = 20, CHGPU_FN_OR = 21, CHGPU_FN_XOR = 22, CHGPU_FN_NOT = 23, /* UInt8 */
    CHGPU_FN_IF = 30,                                                 /* if(cond, then, else): ResultOfIf */
    CHGPU_FN_BIT_AND = 40, CHGPU_FN_BIT_OR = 41, CHGPU_FN_BIT_XOR = 42, /* integers: ResultOfBit */
    CHGPU_FN_TO_YEAR = 50, CHGPU_FN_TO_MONTH = 51, CHGPU_FN_TO_DAY_OF_MONTH = 52, CHGPU_FN_TO_YYYYMM = 53, /* Date -> UInt16/UInt8/UInt8/UInt32 */
    CHGPU_FN_TO_YYYYMMDD = 54, CHGPU_FN_TO_DAY_OF_WEEK = 55, CHGPU_FN_TO_QUARTER = 56, CHGPU_FN_TO_START_OF_MONTH = 57, /* -> UInt32/UInt8/UInt8/Date */
    CHGPU_FN_CAST = 64                                                /* CHGPU_FN_CAST + CHGPU_<type>: toInt64(x) ... (static_cast) */
};
typedef struct chgpu_expr_node
{
    int32_t kind;    /* CHGPU_EX_* */
    int32_t code;    /* INPUT: index into cols[] (< 8); FUNC: CHGPU_FN_*; CONST: unused */
    int32_t type;    /* INPUT, CONST: element type; FUNC: ignored (inferred, see chgpu_expr_node_type) */
    int32_t args[3]; /* FUNC: operand node indices, unused = -1 */
    uint64_t bits;   /* CONST: the value's raw little-endian bytes */
} chgpu_expr_node;
typedef struct chgpu_expr chgpu_expr;
/* type-checks the DAG and generates its row function; needs no device */
int chgpu_expr_compile(uint32_t n_nodes, const chgpu_expr_node * nodes, chgpu_expr ** out);
int chgpu_expr_node_type(const chgpu_expr * expr, uint32_t node, int * type_out);
/* runs the run-time compiler only (no device): n_outputs > 0 -> the materialising kernel for out_nodes (with filter_node >= 0: the
   WHERE + projection pair of chgpu_expr_filter_execute, refused where that call refuses it), n_outputs == 0 -> the fused filter +
   sum kernel for (filter_node, value_node) */
int chgpu_expr_precompile(const chgpu_expr * expr, uint32_t n_outputs, const uint32_t * out_nodes, int filter_node, int value_node,
                          uint64_t * code_bytes_out);
/* materialise out_nodes[n_outputs] (<= 8) as new columns over cols[n_cols] (the INPUT nodes' columns, all of one length) */
int chgpu_expr_execute(chgpu_ctx * ctx, const chgpu_expr * expr, uint32_t n_cols, const chgpu_col * const * cols,
                       uint32_t n_outputs, const uint32_t * out_nodes, chgpu_col ** outs);
/* SELECT sum(value_node), count() WHERE filter_node in one pass, nothing materialised (filter_node < 0: no WHERE;
   value_node < 0: count only).  sum_out: 8 bytes of the SumSimple type of the value node (*result_type_out). */
int chgpu_expr_filter_sum_node(chgpu_ctx * ctx, const chgpu_expr * expr, uint32_t n_cols, const chgpu_col * const * cols,
                               int filter_node, int value_node, int * result_type_out, void * sum_out, uint64_t * count_out);
/* WHERE filter_node + projection of out_nodes (<= 7; INPUT nodes pass columns through) in one step: only the rows whose filter value
   is non-zero are written, in order -- FilterTransform (FilterTransform.cpp:136-256) fused behind the ExpressionTransform, no mask
   and no unfiltered intermediate in HBM.  *rows_out = surviving rows (0: the chunk is dropped; the outputs are empty columns). */
int chgpu_expr_filter_execute(chgpu_ctx * ctx, const chgpu_expr * expr, uint32_t n_cols, const chgpu_col * const * cols,
                              uint32_t filter_node, uint32_t n_outputs, const uint32_t * out_nodes, chgpu_col ** outs,
                              uint64_t * rows_out);
/* SELECT min(value_node), max(value_node), count() WHERE filter_node in one pass (AggregateFunctionMin / Max without key,
   src/AggregateFunctions/AggregateFunctionMinMax.h) for INTEGER value nodes; min_out / max_out receive the value in the node's own
   width (*value_type_out), 0 when no row passes.  Float values -> CHGPU_ERR_NOT_IMPLEMENTED (the reference keeps a NaN that arrives
   first: an order-dependent result). */
int chgpu_expr_filter_minmax_node(chgpu_ctx * ctx, const chgpu_expr * expr, uint32_t n_cols, const chgpu_col * const * cols,
                                  int filter_node, uint32_t value_node, int * value_type_out, void * min_out, void * max_out,
                                  uint64_t * count_out);
int chgpu_expr_free(chgpu_expr * expr);

/* ================================================================================================
 * ASOF joins (JoinStrictness::Asof, INNER and LEFT: joinDispatch.h:66-67).  The reference keeps, per join key, a SortedLookupVector of
 * (asof value, row) and answers a left row with the closest right row under the join's inequality (src/Interpreters/RowRefs.cpp:40-215:
 * insert / findAsof -> boundSearch; HashJoinMethodsImpl.h:462-478).  chgpu_asof is that map for one fixed-width integer key and one numeric
 * asof column: chgpu_asof_add_block = addBlockToJoin (rows with a NULL key, a zero ON mask or a NaN asof value are not inserted), the
 * first probe sorts (the vectors are immutable from then on, RowRefs.cpp:174-178).  chgpu_asof_probe = joinBlock: at most one right row
 * per left row.  INNER: *filter_u8 marks the left rows that found one (need_filter), right_rowid_u64 holds their (block << 32 | row) ids in
 * order, *n_out their number.  LEFT: filter_u8 may be NULL; right_rowid_u64 has one entry per left row, all-ones = the default row
 * (add_missing).  inequality as ASOFJoinInequality (src/Core/Joins.h:78-85) with the LEFT value on the left: GREATER_OR_EQUALS (the
 * default, `a.t >= b.t`) takes the greatest b.t <= a.t.  Right rows with equal (key, asof): the reference's choice is unspecified; here the
 * last inserted for >= / >, the first inserted for <= / <.
 * ============================================================================================== */
enum { CHGPU_ASOF_LESS = 1, CHGPU_ASOF_GREATER = 2, CHGPU_ASOF_LESS_OR_EQUALS = 3, CHGPU_ASOF_GREATER_OR_EQUALS = 4 };
typedef struct chgpu_asof chgpu_asof;
int chgpu_asof_create(chgpu_ctx * ctx, int key_type, int asof_type, int kind, int inequality, chgpu_asof ** out);
int chgpu_asof_add_block(chgpu_asof * join, const chgpu_col * key_col, const chgpu_col * asof_col, const chgpu_col * null_map_u8, const chgpu_col * join_mask_u8,
                         uint64_t * block_index);
int chgpu_asof_total_rows(chgpu_asof * join, uint64_t * rows);
int chgpu_asof_probe(chgpu_asof * join, const chgpu_col * key_col, const chgpu_col * asof_col, const chgpu_col * null_map_u8, chgpu_col ** filter_u8,
                     chgpu_col ** right_rowid_u64, uint64_t * n_out);
int chgpu_asof_free(chgpu_asof * join);

/* ================================================================================================
 * a22 data movement  —  IColumn::index / replicate (src/Columns/ColumnVector.cpp:1121-1143, 879-907)
 * ============================================================================================== */
/* out[i] = col[indexes[i]], i < limit (limit 0 = all); indexes: CHGPU_U64 or CHGPU_U32.
   default_for_missing != 0: index == all-ones (-1) yields the type default 0 (join LEFT misses, insertDefault) */
int chgpu_index(chgpu_ctx * ctx, const chgpu_col * col, const chgpu_col * indexes, uint64_t limit,
                int default_for_missing, chgpu_col ** out);
/* offsets: CHGPU_U64 cumulative (IColumn::Offsets) */
int chgpu_replicate(chgpu_ctx * ctx, const chgpu_col * col, const chgpu_col * offsets_u64, chgpu_col ** out);
/* every column of a Block replicated by one offsets_to_replicate (joinBlock's loop over the left columns,
   src/Interpreters/HashJoin/HashJoinMethodsImpl.h:186-194): one host synchronisation for all of them, columns of one element width share
   a kernel (the offsets are read once).  outs[n_cols] receives the new columns. */
int chgpu_replicate_columns(chgpu_ctx * ctx, uint32_t n_cols, const chgpu_col * const * cols, const chgpu_col * offsets_u64, chgpu_col ** outs);

/* §8(f) rank 4 — ordered output: IColumn::getPermutation(direction, Stable, limit = 0, nan_direction_hint, res) for
   ColumnVector<T> (src/Columns/ColumnVector.cpp:245-330), the step under sortBlock / MergeSortingTransform.  LSD radix sort on
   the device with the stable semantics of less_stable / greater_stable (:120-166): equal values (-0.0 == 0.0, NaN with NaN) keep
   their original order in both directions; NaN is greater than every number when nan_direction_hint > 0, smaller otherwise.
   perm_in_u64 (may be NULL): sort the rows col[perm_in[i]] instead and return the composed permutation -- ORDER BY a, b is
   sort by b, then by a with b's permutation as perm_in.  Apply the result with chgpu_index (IColumn::permute), cut it for LIMIT. */
int chgpu_sort_permutation(chgpu_ctx * ctx, const chgpu_col * col, const chgpu_col * perm_in_u64, int descending,
                           int nan_direction_hint, chgpu_col ** perm_out_u64);

/* getPermutation with a limit (ColumnVector.cpp:254-281: ORDER BY ... LIMIT n): the first `limit` entries of the stable sorted
   permutation.  A threshold from a sorted sample names the candidate rows (one comparison pass + filterToIndices); only they are
   sorted.  Exact; falls back to the full sort when the sample misleads, a value repeats massively or NaNs must come first. */
int chgpu_sort_permutation_limit(chgpu_ctx * ctx, const chgpu_col * col, int descending, int nan_direction_hint, uint64_t limit,
                                 chgpu_col ** perm_out_u64);
/* filterToIndices (src/Columns/ColumnsCommon.cpp:384-470): row numbers whose filter byte is non-zero, ascending */
int chgpu_filter_to_indices(chgpu_ctx * ctx, const chgpu_col * filter_u8, chgpu_col ** indexes_u64, uint64_t * rows_out);

/* Ordered output, the other half: the stable merge of runs that are ALREADY sorted -- MergingSortedAlgorithm
   (src/Processors/Merges/Algorithms/MergingSortedAlgorithm.cpp) over SortCursor (src/Core/SortCursor.h), which is what
   MergeSortingTransform (src/Processors/Transforms/MergeSortingTransform.cpp) does with its sorted chunks, MergingSortedTransform with
   sorted streams and the initiator of a Distributed ORDER BY with the shards' results.
   key_cols[n_keys] (1 to 8, most significant first, any of the ten numeric types) are the runs glued end to end, as chgpu_col_concat
   leaves them; run r is the rows [run_offsets[r], run_offsets[r + 1]) (run_offsets: HOST, n_runs + 1 cumulative entries,
   run_offsets[0] = 0; a run may be empty).  The result is the permutation P of concatenated row numbers for which chgpu_index(col, P)
   is the merged column.  The order of key column j is exactly the one chgpu_sort_permutation(col, .., descending[j],
   nan_direction_hint[j]) defines (-0.0 == 0.0, NaN with NaN, NaN above or below every number by the hint, the complement for
   descending); rows equal on all columns come out by run number, then by row within the run (SortCursor's tie on `order`), that is by
   concatenated row number.  So for runs that are sorted P is bit-equal to the stable sort of the concatenation under the same
   description.  limit > 0: only the first min(limit, rows) entries of P (every run and every merged run is cut to them on the way).
   No rows or no runs: an empty permutation; one run: the identity, cut to the limit.
   flags: CHGPU_MERGE_CHECK_SORTED runs chgpu_is_sorted first and answers BAD_ARGUMENTS naming the row; without it an unsorted run is
   the caller's error and the order is unspecified (nothing is read or written out of bounds).
   Errors: BAD_ARGUMENTS (a NULL ctx, list or output; n_keys of 0 or above 8; an unknown type; offsets that do not start at 0 or
   decrease; unknown flag bits), SIZES_MISMATCH (a key column whose length is not run_offsets[n_runs]), NOT_IMPLEMENTED (2^32 rows or
   more: row numbers travel as UInt32 inside, as in the window operator).  A failed call leaves nothing allocated. */
enum { CHGPU_MERGE_CHECK_SORTED = 1 };
int chgpu_merge_sorted_permutation(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                                   uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint64_t limit, uint32_t flags,
                                   chgpu_col ** perm_out_u64);
/* isAlreadySorted (src/Interpreters/sortBlock.cpp) per run, under the same order and with the same arguments and errors:
   *first_unsorted_row = ~0ull when every run is sorted, else the LOWEST concatenated row number i (not the first of its run) for
   which row i orders strictly before row i - 1.  Rows are never compared across a run boundary.  The same answer in every run. */
int chgpu_is_sorted(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint, uint32_t n_keys,
                    const uint64_t * run_offsets, uint32_t n_runs, uint64_t * first_unsorted_row);

/* The merges of MergeTree that FOLD rows of equal sorting key while they merge -- every background merge of the Replacing / Collapsing /
   Summing / Aggregating engines and every SELECT .. FINAL.  Restated from
   src/Processors/Merges/Algorithms/ReplacingSortedAlgorithm.cpp, src/Processors/Merges/Algorithms/CollapsingSortedAlgorithm.cpp,
   src/Processors/Merges/Algorithms/SummingSortedAlgorithm.cpp and src/Processors/Merges/Algorithms/AggregatingSortedAlgorithm.cpp.
   Common: the arguments up to n_runs and `flags` are those of chgpu_merge_sorted_permutation (1 to 8 numeric key columns over the glued
   runs, at most 2^32 - 1 rows) with n_runs >= 1 -- one run is a merge of a single part -- and no limit; CHGPU_MERGE_CHECK_SORTED is
   honoured.  Rows are visited in the order of that permutation, the merged order M: rows equal on every key come lowest concatenated row
   number first.  A GROUP is a maximal stretch of M whose rows are equal on every key column, equal meaning equal order words
   (hasEqualSortColumnsWith, compareAt(.., 1) == 0: -0.0 = +0.0, NaN = NaN).  Output rows keep M's order and every result is the same bit
   for bit in every run.  An empty input gives empty columns.  Errors as chgpu_merge_sorted_permutation's, before any device work, and
   those named below; a failed call leaves nothing allocated.

   chgpu_merge_replacing: per group the LAST row in M among those with the greatest version (the reference compares with >= 0); without
   a version column (NULL) the group's last row.  version: any integer column, compared in its own signedness; a Float version answers
   NOT_IMPLEMENTED.  is_deleted_u8 (may be NULL; UInt8; without a version NOT_IMPLEMENTED): a value other than 0 or 1 answers
   BAD_ARGUMENTS naming the lowest concatenated row that holds one; with cleanup != 0 a group whose selected row has is_deleted = 1 emits
   nothing.  rows_out_u64: the concatenated row numbers of the selected rows.

   chgpu_merge_collapsing: sign_i8 is Int8; a value other than +1 or -1 answers BAD_ARGUMENTS naming the lowest concatenated row that
   holds it.  Per group cp = the number of +1 rows, cn = the number of -1 rows, first_negative = the first -1 row in M, last_positive =
   the last +1 row in M, last_is_positive = the sign of the group's last row.  Nothing is emitted unless last_is_positive || cp != cn;
   otherwise first_negative if cp <= cn, then last_positive if cp >= cn: 0, 1 or 2 rows, the negative one first.  rows_out_u64: their
   concatenated row numbers.  The reference's log line for |cp - cn| > 1, only_positive_sign have no
   counterpart here.

   chgpu_merge_versioned_collapsing (src/Processors/Merges/Algorithms/VersionedCollapsingAlgorithm.cpp): the engine's sort description
   is the primary key with the version column appended, so the caller passes the version as the LAST key column and a group is a stretch
   equal on the key and the version; there is no separate version argument.  sign_i8 as above.  Within a group the reference keeps a
   queue that only ever holds rows of one sign (sign_in_queue): a row that meets an empty queue sets the sign and is pushed, a row of
   the queue's sign is pushed, a row of the other sign removes the queue's back row and both vanish, and the group's end emits the queue
   front to back.  A group therefore emits |cp - cn| rows, all of the majority sign, in M's order.  Which rows: with B_0 = 0 and
   B_t = B_(t-1) + sign_t over the group's rows in M, row t of sign s survives iff s * B_t >= 1 and s * B_u >= s * B_t for every later row
   u of its group.  rows_out_u64: the concatenated row numbers of the surviving rows, in M's order; empty when everything cancels.
   *max_balance (may be NULL): the largest |B_t| over all rows, 0 for an empty input.  ONE DIFFERENCE: the queue here is unbounded.  The
   reference bounds its queue (max_rows_in_queue, derived from max_block_size) and, when it is full, emits the front row early and for
   good, which makes its output depend on a block-size setting; that bound is not modelled.  The two agree whenever max_balance is below
   the reference's bound, so a caller compares max_balance with its own setting.

   chgpu_merge_folding (Summing; Aggregating over SimpleAggregateFunction columns): value_cols[n_values] with kinds[n_values] of
   CHGPU_FOLD_SUM (wrap-around addition in the column's own type, sumWithOverflow), CHGPU_FOLD_MIN, CHGPU_FOLD_MAX (in the column's
   signedness).  Integer columns only; a Float value column answers NOT_IMPLEMENTED (the reference adds a group's rows one after another
   and a parallel scan rounds differently); more than 8 value columns in one call answer NOT_IMPLEMENTED.  first_rows_u64: the
   concatenated row number of each surviving group's first row in M -- keys and every column the engine does not fold are indexed with
   it (any); last_rows_u64: the same for the group's last row (anyLast); res_cols[n_values]: one result column per value column, in the
   value's type.  drop_zero != 0 is Summing's rule: a group is dropped when n_values > 0 and EVERY SUM result is 0 (with no SUM among the
   kinds that holds for every group); with no value columns nothing is dropped.  SummingMergeTree is every value column SUM with
   drop_zero; AggregatingMergeTree over simple functions is the given kinds without it.  Map / nested summing and AggregateFunction
   state columns are out. */
enum { CHGPU_FOLD_SUM = 0, CHGPU_FOLD_MIN = 1, CHGPU_FOLD_MAX = 2 };
int chgpu_merge_replacing(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                          uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint32_t flags, const chgpu_col * version,
                          const chgpu_col * is_deleted_u8, int32_t cleanup, chgpu_col ** rows_out_u64);
int chgpu_merge_collapsing(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                           uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint32_t flags, const chgpu_col * sign_i8,
                           chgpu_col ** rows_out_u64);
int chgpu_merge_versioned_collapsing(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                                     uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint32_t flags, const chgpu_col * sign_i8,
                                     chgpu_col ** rows_out_u64, uint64_t * max_balance /* may be NULL */);
int chgpu_merge_folding(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                        uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint32_t flags, const chgpu_col * const * value_cols,
                        const int32_t * kinds, uint32_t n_values, int32_t drop_zero, chgpu_col ** first_rows_u64, chgpu_col ** last_rows_u64,
                        chgpu_col ** res_cols);

/* ================================================================================================
 * a11/a21 hashing & sharding  —  ColumnVector::getWeakHash32 (ColumnVector.cpp:78-95), ConcurrentHashJoin
 * hashToSelector (src/Interpreters/ConcurrentHashJoin.cpp:426-440), IColumn::scatter (src/Columns/IColumn.cpp:245-269).
 * Bit-exact CRC32-C (Hash.h:63-66): shard ids are externally visible.
 * ============================================================================================== */
/* hash_u32[i] = (u32) hashCRC32(col[i], hash_u32[i])  (in place; initialise to 0xFFFFFFFF like WeakHash32) */
int chgpu_weak_hash32(chgpu_ctx * ctx, const chgpu_col * col, chgpu_col * hash_u32);
/* selector[i] = ((crc32c(key) >> 24) & 0xFF) & (num_shards-1); num_shards power of two <= 256; out: CHGPU_U32 */
int chgpu_hash_to_selector(chgpu_ctx * ctx, const chgpu_col * keys, uint32_t num_shards, chgpu_col ** selector_u32);
/* stable split of col by selector into num_columns new columns (outs[num_columns]); num_columns <= 256; a selector >= num_columns
 * (a caller bug) counts as 0, so the sizes of the new columns always sum to the rows of col */
int chgpu_scatter(chgpu_ctx * ctx, const chgpu_col * col, const chgpu_col * selector_u32, uint32_t num_columns,
                  chgpu_col ** outs);
/* one-call hash partition of n_cols columns by keys (cols[0] must be the key column or any payload): computes the
   selector once, returns per-shard row counts (host, counts[num_shards]) and for each input column ONE output column
   holding the shards back to back (shard s occupies [sum(counts[:s]), +counts[s])) — the send buffer of an
   all-to-all.  Stable within a shard. */
int chgpu_partition_by_hash(chgpu_ctx * ctx, const chgpu_col * keys, uint32_t num_shards, uint32_t n_cols,
                            const chgpu_col * const * cols, chgpu_col ** outs, uint64_t * counts);

/* ================================================================================================
 * a12-a17 GROUP BY  —  Aggregator::executeOnBlock / mergeOnBlock / convertToBlocks
 * (src/Interpreters/Aggregator.h:179-190,227,253; Aggregator.cpp:1506-1627, 2468-2725, 2037-2117) with
 * AggregatedDataVariants key32/key64 = HashMap<UInt64, AggregateDataPtr> (AggregatedData.h:38).
 * One chgpu_agg == one AggregatedDataVariants (single writer).  key_type < 0: without_key.
 * Device table: open addressing, linear probing, power-of-two capacity, max fill 1/2, growth x4 until 2^23 then x2,
 * empty <=> key == 0 with the zero key kept out of line — the geometry of HashTable.h:217-330,358-391.
 * ============================================================================================== */
/* a15 multi-column fixed-width keys: packFixed<UInt64> (src/Interpreters/AggregationCommon.h:91-158) — the keys16/32/64
   variants of chooseAggregationMethod (Aggregator.cpp:773-778).  Columns are laid out consecutively (little endian) in one
   UInt64 per row; more than 8 key bytes -> CHGPU_ERR_NOT_IMPLEMENTED here: use a chgpu_keydict (keys128 / keys256, below).  unpack is the
   inverse used when the key column(s) of the result block are produced (insertKeyIntoColumns). */
int chgpu_pack_fixed_keys(chgpu_ctx * ctx, uint32_t n_cols, const chgpu_col * const * cols, chgpu_col ** packed_u64);
int chgpu_unpack_fixed_key(chgpu_ctx * ctx, const chgpu_col * packed_u64, uint32_t byte_offset, int type, chgpu_col ** out);
/* FixedString(N) keys (ColumnFixedString: rows x N raw bytes, src/Columns/ColumnFixedString.h; AggregatedDataVariants::key_fixed_string,
   AggregatedDataVariants.h:65-66,91-92; HashJoin key_fixed_string).  A value is N bytes, padding zeros included: a fixed-width key.  Word w =
   bytes [8w, 8w + 8) of every value as one UInt64 (little endian, zero padded past N): N <= 8 -> the ordinary UInt64 key (key64), N <= 32 ->
   keys128 / keys256 (chgpu_keydict_*).  chgpu_fixed_string_from_words is insertKeyIntoColumns: words -> chars.  N > 32 -> NOT_IMPLEMENTED. */
int chgpu_fixed_string_word(chgpu_ctx * ctx, const chgpu_col * chars_u8, uint32_t n, uint32_t word_index, chgpu_col ** out_u64);
int chgpu_fixed_string_from_words(chgpu_ctx * ctx, uint32_t n_words, const chgpu_col * const * words_u64, uint32_t n, chgpu_col ** chars_u8);
/* a15 keys128 / keys256: several fixed-width key columns that pack into more than 8 bytes (AggregatedDataVariants.h:70-71,83-84:
   HashMap<UInt128 / UInt256, ...>; HashMethodKeysFixed, src/Common/ColumnsHashing/HashMethod.h:236-410; packFixed,
   AggregationCommon.h:91-158; the same maps under HashJoin, HashJoin.h:267-358).  A chgpu_keydict is a device-resident, exact dictionary
   packed key -> dense UInt32 id (numbered as keys are first claimed; stable for the dictionary's lifetime, across blocks and growth).
   chgpu_keydict_encode packs the columns of rows [row_begin, row_end) (packFixed order: consecutively, little endian, zero padded to
   key_bytes = 16 or 32) and returns their ids: insert != 0 is emplaceKey (GROUP BY, join build), insert == 0 is findKey (join probe):
   a key the dictionary does not hold gets 0xFFFFFFFF.  The ids are an ordinary UInt32 key column for chgpu_agg_* / chgpu_join_* /
   chgpu_partition_*; chgpu_keydict_key_column gives back one original key column for a column of ids (insertKeyIntoColumns; bytes
   [byte_offset, +sizeof(type)) of the packed key; 0xFFFFFFFF -> 0); chgpu_keydict_selector the shard of every id by the reference's own
   hash of the packed key (UInt128HashCRC32 / UInt256HashCRC32, Hash.h:346-355,412-423 -> two-level bucket & (num_shards - 1)). */
typedef struct chgpu_keydict chgpu_keydict;
int chgpu_keydict_create(chgpu_ctx * ctx, uint32_t key_bytes, uint64_t size_hint, chgpu_keydict ** out);
int chgpu_keydict_encode(chgpu_keydict * dict, uint32_t n_cols, const chgpu_col * const * cols, uint64_t row_begin, uint64_t row_end, int insert,
                         chgpu_col ** ids_u32);
int chgpu_keydict_size(chgpu_keydict * dict, uint64_t * n_keys);
int chgpu_keydict_key_column(chgpu_keydict * dict, const chgpu_col * ids_u32, uint32_t byte_offset, int type, chgpu_col ** out);
int chgpu_keydict_selector(chgpu_keydict * dict, const chgpu_col * ids_u32, uint32_t num_shards, chgpu_col ** selector_u32);
int chgpu_keydict_free(chgpu_keydict * dict);
/* uniqExact(x) / count(DISTINCT x) under GROUP BY (AggregateFunctionUniqExact: a HashSet<T> per group; count_distinct_implementation =
   uniqExact).  A chgpu_uniq is ONE exact set of (group key, value) pairs in HBM, beside the chgpu_agg that holds the GROUP BY's other
   aggregates: one chgpu_uniq per distinct-counted argument.
   Types: key_type is an integer type (zero-extended to the UInt64 table key as for chgpu_agg; ids of chgpu_keydict_* / chgpu_lc_remap /
   the String dictionary and keys of chgpu_pack_fixed_keys are ordinary UInt32 / UInt64 keys), a float key answers
   CHGPU_ERR_NOT_IMPLEMENTED, key_type < 0 is without key; value_type is any of the ten types.  Two values are equal when their bits are
   (the HashSet cell's bitEquals): +0.0 and -0.0 are two values, NaNs with one payload are one, Float32 is compared as its 32 bits.
   Every bit pattern is a legal key and a legal value.  size_hint: distinct pairs expected, 0 = unknown (the table grows).
   chgpu_uniq_add_block: rows [row_begin, row_end) whose filter_u8 byte is non-zero enter (filter_u8 may be NULL: every row).  The filter
   is WHERE, the -If condition and the negated null map in one byte (chgpu_and / chgpu_filter_description_nullable), so uniqExactIf and a
   Nullable argument are this same call.  A group exists only through a row that entered.  key_col is ignored without key.
   chgpu_uniq_merge: set union, src stays valid; both of one (key_type, value_type) and on one device.
   chgpu_uniq_size: distinct pairs held.
   chgpu_uniq_export_pairs: the not-final form -- every distinct pair once, as a key column and a value column of the set's types, order
   unspecified; a peer merges them with chgpu_uniq_add_block, a sharded GROUP BY routes them with chgpu_partition_by_hash on the key
   column.  Without key keys_out may be NULL (it receives NULL).
   chgpu_uniq_finalize: one row per key that has a pair -- the key and the UInt64 count of its distinct values, order unspecified;
   without key exactly one row (0 for the empty set; keys_out may be NULL).  May be called repeatedly and between blocks.
   chgpu_uniq_counts_for_keys: for every row of `keys` (the set's key type) that key's distinct count, 0 for a key the set lacks: the
   uniqExact column beside the columns of chgpu_agg_finalize, in that call's row order.
   Errors: NULL handles and outputs, type mismatches, row_begin > row_end, a range past the column, sets of different types or devices ->
   CHGPU_ERR_BAD_ARGUMENTS; columns of different lengths -> CHGPU_ERR_SIZES_MISMATCH; more than 2^31 distinct pairs ->
   CHGPU_ERR_TOO_MANY_ROWS; after CHGPU_ERR_OOM the set holds exactly what it held before the call.  Empty inputs are not errors.
   The reference's wire bytes (HashSet::write per group) are not produced. */
typedef struct chgpu_uniq chgpu_uniq;
int chgpu_uniq_create(chgpu_ctx * ctx, int key_type, int value_type, uint64_t size_hint, chgpu_uniq ** out);
int chgpu_uniq_add_block(chgpu_uniq * uniq, const chgpu_col * key_col, const chgpu_col * value_col, uint64_t row_begin, uint64_t row_end,
                         const chgpu_col * filter_u8);
int chgpu_uniq_merge(chgpu_uniq * dst, const chgpu_uniq * src);
int chgpu_uniq_size(chgpu_uniq * uniq, uint64_t * pairs);
int chgpu_uniq_export_pairs(chgpu_uniq * uniq, chgpu_col ** keys_out, chgpu_col ** values_out, uint64_t * pairs);
int chgpu_uniq_finalize(chgpu_uniq * uniq, chgpu_col ** keys_out, chgpu_col ** counts_u64, uint64_t * groups);
int chgpu_uniq_counts_for_keys(chgpu_uniq * uniq, const chgpu_col * keys, chgpu_col ** counts_u64);
int chgpu_uniq_free(chgpu_uniq * uniq);
/* quantileExact / quantilesExact / medianExact and their Low / High forms under GROUP BY (AggregateFunctionQuantile over QuantileExact:
   an array of the values per group, push_back at add, nth_element at the end).  A chgpu_quantile holds the multiset of (group key,
   value) pairs in one flat append-only store in HBM, beside the chgpu_agg that holds the GROUP BY's other aggregates: one per argument.
   Adding a block is a filtered copy; finalising scatters the values into per-group segments and selects the requested ranks (short
   segments sorted in LDS, long ones by byte-wise histogram passes).  Levels and kind belong to finalize / for_keys: one state serves
   any of them, repeatedly and between blocks.
   Types: keys as for chgpu_uniq (integer types, zero-extended; a float key answers CHGPU_ERR_NOT_IMPLEMENTED; key_type < 0 is without
   key); value_type is any of the ten types.
   What enters: a row of [row_begin, row_end) whose filter_u8 byte is non-zero (NULL: every row) and whose value is not NaN.  +-inf,
   denormals and -0.0 are ordinary values.  A group exists only through a row that entered.
   Rank: for a level l in [0, 1] and a group of n >= 1 values the answer is the element of 0-based rank r in ascending order:
     CHGPU_QUANTILE_EXACT       r = l < 1 ? (uint64_t)(l * (double)n) : n - 1        (one IEEE double product, truncated)
     CHGPU_QUANTILE_EXACT_LOW   l == 0.5: r = n odd ? n / 2 : n / 2 - 1; else as EXACT
     CHGPU_QUANTILE_EXACT_HIGH  l == 0.5: r = n / 2; else as EXACT
   The result has the value's type and is one of the group's elements bit for bit; the order is numeric with -0.0 directly before +0.0.
   An empty state (a key the operator lacks in for_keys, the without-key operator with no value) gives quiet NaN for floats, 0 for
   integers.  The reserved kinds (Inclusive, Exclusive, Weighted) answer CHGPU_ERR_NOT_IMPLEMENTED.
   chgpu_quantile_merge: multiset union, src stays valid.  chgpu_quantile_size: values held, all groups.
   chgpu_quantile_export_pairs: the not-final form -- every held value with its key, order unspecified; a peer takes them with
   chgpu_quantile_add_block, a sharded GROUP BY routes them with chgpu_partition_by_hash.  Without key keys_out may be NULL.
   chgpu_quantile_finalize: one row per key that holds a value, order unspecified, res_cols[i] answers levels[i]; without key exactly
   one row (keys_out may be NULL).  chgpu_quantile_for_keys: for every row of `keys` that key's quantiles: the columns beside those of
   chgpu_agg_finalize, in that call's row order.
   Errors: NULL handles and outputs, type mismatches, row_begin > row_end, a range past the column, n_levels == 0 or above
   CHGPU_QUANTILE_MAX_LEVELS, a level outside [0, 1] or NaN, operators of different types or devices -> CHGPU_ERR_BAD_ARGUMENTS; columns
   of different lengths -> CHGPU_ERR_SIZES_MISMATCH; 2^32 - 1 values or more -> CHGPU_ERR_TOO_MANY_ROWS; after CHGPU_ERR_OOM the state
   holds exactly what it held before the call.  Empty inputs are not errors.  The reference's wire bytes are not produced. */
enum { CHGPU_QUANTILE_EXACT = 0, CHGPU_QUANTILE_EXACT_LOW = 1, CHGPU_QUANTILE_EXACT_HIGH = 2,
       CHGPU_QUANTILE_EXACT_INCLUSIVE = 3, CHGPU_QUANTILE_EXACT_EXCLUSIVE = 4, CHGPU_QUANTILE_EXACT_WEIGHTED = 5 /* 3..5: reserved */ };
#define CHGPU_QUANTILE_MAX_LEVELS 16
typedef struct chgpu_quantile chgpu_quantile;
int chgpu_quantile_create(chgpu_ctx * ctx, int key_type, int value_type, chgpu_quantile ** out);
int chgpu_quantile_add_block(chgpu_quantile * quantile, const chgpu_col * key_col, const chgpu_col * value_col, uint64_t row_begin, uint64_t row_end,
                             const chgpu_col * filter_u8);
int chgpu_quantile_merge(chgpu_quantile * dst, const chgpu_quantile * src);
int chgpu_quantile_size(chgpu_quantile * quantile, uint64_t * values);
int chgpu_quantile_export_pairs(chgpu_quantile * quantile, chgpu_col ** keys_out, chgpu_col ** values_out, uint64_t * rows);
int chgpu_quantile_finalize(chgpu_quantile * quantile, int kind, uint32_t n_levels, const double * levels, chgpu_col ** keys_out,
                            chgpu_col ** res_cols, uint64_t * groups);
int chgpu_quantile_for_keys(chgpu_quantile * quantile, int kind, uint32_t n_levels, const double * levels, const chgpu_col * keys,
                            chgpu_col ** res_cols);
int chgpu_quantile_free(chgpu_quantile * quantile);
/* groupArray(x) / groupArray(N)(x) under GROUP BY (AggregateFunctionGroupArray over GroupArrayNumericImpl: an array per group, push_back
   at add until max_elems, insert(end, rhs...) at merge).  A chgpu_group_array holds the (group key, value) pairs in one flat append-only
   store in HBM IN ARRIVAL ORDER, beside the chgpu_agg that holds the GROUP BY's other aggregates: one per argument.  Adding a block is an
   order-preserving filtered copy; finalising runs one stable radix pass per key byte that varies anywhere in the store, which leaves
   equal keys adjacent and every group's values in arrival order, and hands the result out as a ColumnArray in two columns.
   Types: keys as for chgpu_uniq / chgpu_quantile (integer types, zero-extended; a float key answers CHGPU_ERR_NOT_IMPLEMENTED; key_type
   < 0 is without key); value_type is any of the ten types (UInt32 dictionary ids stand for a LowCardinality / String argument).
   max_size: N of groupArray(N), 0 = no limit.
   What enters: a row of [row_begin, row_end) whose filter_u8 byte is non-zero (NULL: every row); the filter is WHERE, the -If condition
   and the negated null map in one byte, so groupArrayIf and a Nullable argument are this same call.  Nothing else is dropped: NaN of
   any payload, +-inf and -0.0 are kept and every value comes back bit for bit.  A group exists only through a row that entered.
   Order: a group's array holds its entered values by add_block call, then by row number within the call.  chgpu_group_array_merge puts
   src's values behind dst's, src stays valid.  With max_size = N > 0 an array is the first N of that sequence (the reference's "stop
   adding at N" and "take N - size from rhs"); the store still keeps every entered row.  Operators of different max_size do not merge.
   The reference's order under several threads depends on their timing; this operator's order is fully determined by the calls.
   Result: offsets_u64[i] is where array i ends (ColumnArray::getOffsets): array i is data[offsets[i - 1], offsets[i]) with offsets[-1]
   = 0; data_out has the value type.  chgpu_group_array_finalize: one row per key that holds a value, the keys in the key type, row
   order unspecified but the same across calls on an unchanged store; without key exactly one row, which may be the empty array
   (keys_out may be NULL).  chgpu_group_array_for_keys: for every row of `keys` that key's array, in that call's row order: the column
   beside those of chgpu_agg_finalize; a key the operator lacks gets the empty array, a key asked twice gets its array twice.
   chgpu_group_array_export_pairs: the not-final form -- every held pair IN STORE ORDER; a peer that feeds them to
   chgpu_group_array_add_block rebuilds the same arrays.  chgpu_group_array_size: values held, all groups.  finalize and for_keys may be
   called repeatedly and between blocks.
   Errors: NULL handles and outputs, type mismatches, row_begin > row_end, a range past the column, operators of different types,
   max_size or devices -> CHGPU_ERR_BAD_ARGUMENTS; columns of different lengths -> CHGPU_ERR_SIZES_MISMATCH; 2^32 - 1 values or more ->
   CHGPU_ERR_TOO_MANY_ROWS; after CHGPU_ERR_OOM the store holds exactly what it held before the call.  Empty inputs are not errors.  The
   reference's wire bytes (VarUInt size + raw values per group) are not produced. */
typedef struct chgpu_group_array chgpu_group_array;
int chgpu_group_array_create(chgpu_ctx * ctx, int key_type, int value_type, uint64_t max_size, chgpu_group_array ** out);
int chgpu_group_array_add_block(chgpu_group_array * group_array, const chgpu_col * key_col, const chgpu_col * value_col, uint64_t row_begin,
                                uint64_t row_end, const chgpu_col * filter_u8);
int chgpu_group_array_merge(chgpu_group_array * dst, const chgpu_group_array * src);
int chgpu_group_array_size(chgpu_group_array * group_array, uint64_t * values);
int chgpu_group_array_export_pairs(chgpu_group_array * group_array, chgpu_col ** keys_out, chgpu_col ** values_out, uint64_t * rows);
int chgpu_group_array_finalize(chgpu_group_array * group_array, chgpu_col ** keys_out, chgpu_col ** offsets_u64, chgpu_col ** data_out,
                               uint64_t * groups);
int chgpu_group_array_for_keys(chgpu_group_array * group_array, const chgpu_col * keys, chgpu_col ** offsets_u64, chgpu_col ** data_out);
int chgpu_group_array_free(chgpu_group_array * group_array);
/* SELECT DISTINCT and LIMIT n [OFFSET m] BY key: DistinctTransform and LimitByTransform::transform
   (src/Processors/Transforms/DistinctTransform.cpp, LimitByTransform.cpp), with exact keys in place of their SipHash128 of the key
   columns.  Both clauses ask one thing of a row: how many earlier rows, over all blocks so far and in row order, had this key.  A
   chgpu_limit_by keeps a key -> counter table in HBM across calls and answers a block with an ordinary IColumn::Filter (UInt8, 0 / 1)
   for chgpu_filter_columns, chgpu_string_filter and ColumnLowCardinality.filter.
   Semantics: walk the rows of [row_begin, row_end) in row order.  A row whose filter_u8 byte is zero (NULL: no such row; WHERE fused in,
   as in chgpu_uniq_add_block) gets 0 and counts nowhere.  Any other row reads its key's counter c: if c < group_offset + group_length
   the counter becomes c + 1 and the row passes iff c >= group_offset; else the row gets 0.  Counters persist over calls.  DISTINCT is
   group_length = 1, group_offset = 0.  out_filter_u8 has row_end - row_begin bytes, *rows_passed is their sum (a transform drops an
   empty chunk and passes a full one untouched).  The result is fully determined by the calls: the same in every run.
   Keys: key_type is an integer type of 1-8 bytes, its raw bits zero-extended as for chgpu_agg and chgpu_uniq; every bit pattern is a
   legal key, 0 and 2^64 - 1 included.  A float key and key_type < 0 (without a key the clause is a plain LIMIT) answer
   CHGPU_ERR_NOT_IMPLEMENTED.  Ids from chgpu_keydict_*, chgpu_lc_remap and the String dictionary, and packed keys, are ordinary keys.
   size_hint: expected number of keys (0: the table starts small and grows).  chgpu_limit_by_keys: keys counted at least once.
   Errors: NULL handle or outputs, group_length == 0, row_begin > row_end, a range past the column, a key column of another type ->
   CHGPU_ERR_BAD_ARGUMENTS; a filter of another length than the key column -> CHGPU_ERR_SIZES_MISMATCH; group_offset + group_length >
   2^32 - 1 (counters are 32-bit and saturate at that sum) -> CHGPU_ERR_NOT_IMPLEMENTED; 2^32 rows or more in one call, or more
   than 2^30 keys (a slot is a 32-bit cell index of a table at most half full) -> CHGPU_ERR_TOO_MANY_ROWS.  After CHGPU_ERR_OOM every counter holds what it held before the call (keys the failed
   call inserted may stay with counter 0, which is what an absent key has).  An empty range is not an error: empty filter, 0 passed. */
typedef struct chgpu_limit_by chgpu_limit_by;
int chgpu_limit_by_create(chgpu_ctx * ctx, int key_type, uint64_t group_length, uint64_t group_offset, uint64_t size_hint, chgpu_limit_by ** out);
int chgpu_limit_by_filter_block(chgpu_limit_by * lb, const chgpu_col * key_col, uint64_t row_begin, uint64_t row_end,
                                const chgpu_col * filter_u8 /* may be NULL */, chgpu_col ** out_filter_u8, uint64_t * rows_passed);
int chgpu_limit_by_keys(chgpu_limit_by * lb, uint64_t * keys);   /* keys that have been counted at least once */
int chgpu_limit_by_free(chgpu_limit_by * lb);                    /* NULL is OK */
/* Window functions over a sorted block: WindowTransform (src/Processors/Transforms/WindowTransform.cpp: advancePartitionEnd,
   advanceFrameStart / advanceFrameEnd, arePeers; the functions WindowFunctionRowNumber, WindowFunctionRank, WindowFunctionDenseRank,
   WindowFunctionLagLeadInFrame and the aggregate functions run over a frame) with the frames of src/Interpreters/WindowDescription.h
   (WindowFrame: FrameType, BoundaryType, checkValid).  `OVER (PARTITION BY p.. ORDER BY o.. ROWS|RANGE ..)` behind the sort this library
   already does: the input is the WHOLE sorted input, the columns as chgpu_sort_permutation + chgpu_index leave them, at most 2^32 - 1
   rows (more -> CHGPU_ERR_NOT_IMPLEMENTED).  There is no carry between blocks: a frame that looks ahead needs rows not yet seen, so a
   caller glues its chunks with chgpu_col_concat first.
   One handle is one window definition (WINDOW w AS (..)).  chgpu_window_create reads the key columns once and keeps only what it derives
   from them -- a flag byte per row and, built on the first call that reads them, the rows' partition and peer-group bounds; it holds no
   reference to the keys.  Each list holds 0 to 8 columns of any of the ten types (String / LowCardinality keys as dictionary ids);
   n_partition = 0 is one partition, n_order = 0 makes all rows of a partition peers.  Row i starts a partition when i = 0 or a partition
   column differs from row i - 1, and a peer group when it starts a partition or an order column differs; equality is compareAt == 0:
   integers by value, floats with a == b or both NaN (so -0.0 equals +0.0).  [ps, pe) is the partition of row i, [gs, ge) its peer group.
   chgpu_window_evaluate computes one function OVER w; several calls share a handle, each with its own frame (NULL: the reference's
   default, RANGE UNBOUNDED PRECEDING .. CURRENT ROW).  The frame [fs, fe) of row i, all arithmetic saturating:
     bound                  begin                 end
     UNBOUNDED_PRECEDING    ps                    BAD_ARGUMENTS
     OFFSET_PRECEDING k     max(ps, i - k)        max(ps, i - k + 1)
     CURRENT_ROW            ROWS i, RANGE gs      ROWS i + 1, RANGE ge
     OFFSET_FOLLOWING k     min(pe, i + k)        min(pe, i + k + 1)
     UNBOUNDED_FOLLOWING    BAD_ARGUMENTS         pe
   CURRENT_ROW .. k PRECEDING, k FOLLOWING .. CURRENT_ROW / m PRECEDING, k PRECEDING .. m PRECEDING with k < m and k FOLLOWING .. m
   FOLLOWING with k > m are CHGPU_ERR_BAD_ARGUMENTS (WindowFrame::checkValid); a frame may be empty.  RANGE with an offset ->
   CHGPU_ERR_NOT_IMPLEMENTED.  `reserved` is ignored.
     function        arg               result          value
     ROW_NUMBER      -                 UInt64          i - ps + 1                          (frame ignored)
     RANK            -                 UInt64          gs - ps + 1                         (frame ignored)
     DENSE_RANK      -                 UInt64          peer groups in [ps, i]              (frame ignored)
     COUNT           -                 UInt64          fe - fs
     SUM             8 integer types   Int64 / UInt64  wrap-around sum of the frame (SumSimple's result type)
     AVG             8 integer types   Float64         that sum as Float64 / Float64(fe - fs), as CHGPU_AGG_AVG; empty frame: NaN
     MIN / MAX       all ten           arg type        extremum in the order of chgpu_agg's min / max (NaN in its total-order place, +0.0
                                                       above -0.0, the value's bits returned); empty frame: 0.  The frame must begin
                                                       UNBOUNDED_PRECEDING or end UNBOUNDED_FOLLOWING, else CHGPU_ERR_NOT_IMPLEMENTED
     FIRST_VALUE     all ten           arg type        x[fs], bits untouched; empty frame: 0
     LAST_VALUE      all ten           arg type        x[fe - 1], bits untouched; empty frame: 0
     LAG_IN_FRAME    all ten           arg type        t = i - offset: x[t] if fs <= t < fe, else default_bits narrowed to the type
     LEAD_IN_FRAME   all ten           arg type        t = i + offset, likewise; offset 0 is the row itself, nothing wraps
   SUM / AVG over Float32 / Float64 -> CHGPU_ERR_NOT_IMPLEMENTED.  `arg` must be NULL where the function takes none; `offset` and
   `default_bits` are read by lag / lead only.  *out is a new column of `rows` rows, caller frees.
   chgpu_window_counts: the rows, partitions and peer groups of the handle (any pointer may be NULL).
   Errors: NULL handles, lists and outputs, more than 8 columns in a list, an unknown function, bound or type, an illegal frame, a missing
   or surplus arg -> CHGPU_ERR_BAD_ARGUMENTS; a key column or arg whose length is not `rows` -> CHGPU_ERR_SIZES_MISMATCH.  A failed call
   leaves nothing allocated and the handle usable.  Nullable keys and arguments, GROUPS frames, nth_value, ntile, percent_rank and
   lag / lead without InFrame are not provided. */
typedef struct chgpu_window chgpu_window;
enum { CHGPU_WIN_ROW_NUMBER = 0, CHGPU_WIN_RANK, CHGPU_WIN_DENSE_RANK, CHGPU_WIN_COUNT, CHGPU_WIN_SUM, CHGPU_WIN_AVG,
       CHGPU_WIN_MIN, CHGPU_WIN_MAX, CHGPU_WIN_FIRST_VALUE, CHGPU_WIN_LAST_VALUE, CHGPU_WIN_LAG_IN_FRAME, CHGPU_WIN_LEAD_IN_FRAME };
enum { CHGPU_FRAME_ROWS = 0, CHGPU_FRAME_RANGE = 1 };
enum { CHGPU_BOUND_UNBOUNDED_PRECEDING = 0, CHGPU_BOUND_OFFSET_PRECEDING, CHGPU_BOUND_CURRENT_ROW,
       CHGPU_BOUND_OFFSET_FOLLOWING, CHGPU_BOUND_UNBOUNDED_FOLLOWING };
typedef struct { int32_t type, begin_kind, end_kind, reserved; uint64_t begin_offset, end_offset; } chgpu_window_frame;
int chgpu_window_create(chgpu_ctx * ctx, const chgpu_col * const * partition_cols, uint32_t n_partition,
                        const chgpu_col * const * order_cols, uint32_t n_order, uint64_t rows, chgpu_window ** out);
int chgpu_window_counts(chgpu_window * window, uint64_t * rows, uint64_t * partitions, uint64_t * peer_groups);
int chgpu_window_evaluate(chgpu_window * window, int function, const chgpu_window_frame * frame /* NULL = default */,
                          const chgpu_col * arg /* NULL where the function takes none */,
                          uint64_t offset /* lag / lead */, uint64_t default_bits /* lag / lead */, chgpu_col ** out);
int chgpu_window_free(chgpu_window * window);
/* chgpu_window_evaluate_framed: chgpu_window_evaluate plus the two kinds of frame it refuses.  Everything chgpu_window_evaluate serves
   is served here with the same results bit for bit (the same code runs), with `order` NULL.  On top of that:
   (a) MIN / MAX over every legal frame, ROWS or RANGE: bounded on both sides, not containing the current row (5 PRECEDING .. 2
       PRECEDING), empty (-> 0).  The extremum is taken in the order of chgpu_agg's min / max as above (NaN in its total-order place, +0.0
       above -0.0) and the value's bits are returned.  A frame that begins UNBOUNDED_PRECEDING or ends UNBOUNDED_FOLLOWING keeps the
       running extremum; every other one reads a 64-bit mask per row (the monotone stack of the row's 64-row block) and a sparse table
       over the blocks' extrema: a few gathers per row whatever the frame's width.
   (b) RANGE frames with OFFSET_PRECEDING / OFFSET_FOLLOWING bounds for COUNT, SUM, AVG, MIN, MAX, FIRST_VALUE, LAST_VALUE, LAG_IN_FRAME
       and LEAD_IN_FRAME.  `order` is the window's one ORDER BY column x, sorted as it was given to chgpu_window_create, `descending` its
       direction (0: ASC, 1: DESC; read only with `order`).  All arithmetic on values is exact, as if in unbounded integers: x[i] - k may
       lie below the type's minimum (every row is >= it) and x[i] + k above its maximum (no row is) -- compareValuesWithOffset's overflow
       branches.  Ascending, [ps, pe) the partition of row i:
         bound           begin fs = first j in [ps, pe) with .. (else pe)    end fe = first j in [ps, pe) with .. (else pe)
         k PRECEDING     x[j] >= x[i] - k                                    x[j] > x[i] - k
         CURRENT_ROW     gs                                                  ge
         k FOLLOWING     x[j] >= x[i] + k                                    x[j] > x[i] + k
         UNBOUNDED       ps                                                  pe
       Descending: the same over the negated values (k PRECEDING begins at the first j with x[j] <= x[i] + k).  An offset of 0 gives
       gs / ge.  The legality rules are those above; a legal frame has fs <= fe.  `order` is one of the eight integer types; a
       Float32 / Float64 order column -> CHGPU_ERR_NOT_IMPLEMENTED.  The handle must have been created with exactly one ORDER BY column
       of that type and length (create records the count and the type, no reference to the keys).
   Errors beyond those of chgpu_window_evaluate: NULL `order` with a RANGE frame that has an offset, `order` given with any other frame
   (or with a function that ignores the frame), a handle created with 0 or >= 2 order columns, an order column whose type differs from
   the one recorded at create -> CHGPU_ERR_BAD_ARGUMENTS; an order column of another length -> CHGPU_ERR_SIZES_MISMATCH.  That `order`
   is the column the handle was created with, sorted that way, is not checked: if it is not sorted within its partitions the results
   are unspecified, but every index a kernel forms stays inside [ps, pe] and every loop ends.  SUM / AVG over Float32 / Float64 stay
   CHGPU_ERR_NOT_IMPLEMENTED, GROUPS frames and the rest of the list above stay not provided.  A failed call allocates nothing and leaves
   the handle usable; *out is as for chgpu_window_evaluate.  The searched bounds are a call's temporaries, not kept in the handle. */
int chgpu_window_evaluate_framed(chgpu_window * window, int function, const chgpu_window_frame * frame /* NULL = default */,
                                 const chgpu_col * order /* the one ORDER BY column; required by a RANGE frame with an offset, else NULL */,
                                 int descending /* 0: ORDER BY o ASC, 1: DESC; read only with `order` */,
                                 const chgpu_col * arg, uint64_t offset, uint64_t default_bits, chgpu_col ** out);
/* §8(f) rank 2 — LowCardinality keys (src/Columns/ColumnLowCardinality.h:27-69; low_cardinality_key* variants,
   AggregatedDataVariants.h:119-127; HashMethodSingleLowCardinalityColumn's per-position cache, ColumnsHashing.h:82-260).
   Every Block brings its own dictionary; the host resolves it against the query-wide dictionary into remap_u32[local position]
   = global id, and the rows are translated on the device: out_u32[i] = remap_u32[indexes[i]] (indexes: UInt8/16/32/64).
   The result is an ordinary UInt32 key column for chgpu_agg_* / chgpu_join_* / chgpu_hash_to_selector. */
int chgpu_lc_remap(chgpu_ctx * ctx, const chgpu_col * indexes, const chgpu_col * remap_u32, chgpu_col ** out_u32);
/* §8(f) rank 2 — String keys.  ColumnString (src/Columns/ColumnString.h:40-49) = chars_u8 (every value followed by a zero byte) +
   offsets_u64 (offsets[i] = end of value i including that zero).  Every row gets the dense id of its value, ids numbered by
   first appearance (ColumnUnique::uniqueInsertRangeFrom, src/Columns/ColumnUnique.h:520-620); first_rows_u64[id] = the row where
   the value first appears (the caller reads the dictionary's strings from its own Block there).  Exact: values are compared
   byte by byte; a 64-bit tag shared by two different values answers CHGPU_ERR_NOT_IMPLEMENTED (CPU path).  ids + dictionary
   are a ColumnLowCardinality: chgpu_lc_remap / GROUP BY / join as above.  The kernels read values 8 bytes at a time: a wrapped chars
   buffer (chgpu_col_wrap) must keep 8 readable bytes after its end, as PaddedPODArray's right pad does (columns made by this library do). */
int chgpu_string_dictionary_encode(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, chgpu_col ** ids_u32,
                                   chgpu_col ** first_rows_u64, uint64_t * n_distinct);
/* ColumnString::filter (src/Columns/ColumnString.cpp:270-290 -> filterArraysImpl, src/Columns/ColumnsCommon.cpp:191-286): the values
   whose filter byte is non-zero, in order, as a new ColumnString (offsets rebuilt, bytes moved together). */
int chgpu_string_filter(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, const chgpu_col * filter_u8,
                        chgpu_col ** out_offsets_u64, chgpu_col ** out_chars_u8, uint64_t * rows_out);
/* §8(f) rank 4 over Strings -- ColumnString::getPermutation(direction, Stable, limit, ...) without collation (src/Columns/ColumnString.cpp),
   the String half of sortBlock.  Order: values compare as UNSIGNED bytes over the first min(len_a, len_b) bytes, then the shorter value is
   the smaller one; lengths exclude the terminating zero (the rule of chgpu_string_cmp_const).  Binary-safe: zero bytes and bytes >= 0x80
   inside values are ordinary bytes, "ab" < "ab\0" < "ab\0\0" < "ab\1".  Stable: equal values keep their incoming order in both directions
   (descending reverses the comparison, not the row order among ties); the incoming order is row order, or perm_in order when perm_in is
   given -- the permutation is unique.  perm_in_u64 (may be NULL) as in chgpu_sort_permutation: sort the rows perm_in[i] and return the
   composed permutation, so ORDER BY a, s is "sort by s, then stably by a" with either kind of column in either place; perm_in.rows > rows
   answers CHGPU_ERR_SIZES_MISMATCH, an entry >= rows is treated as row 0 and never faults.  limit (0 = none): with 0 < limit < n the
   result has `limit` rows, exactly the first `limit` entries of the full stable permutation (also with perm_in: the most significant
   column of a description can take the query's LIMIT).  An MSD sort in 8-byte words, every round the stable radix passes of
   chgpu_sort_permutation over the rows still undecided; a prefix shared by all rows of a tie costs no rounds.
   Offsets that break the ColumnString invariant answer CHGPU_ERR_BAD_ARGUMENTS, as do wrong column types and NULL arguments; zero rows
   give an empty column; chars needs the same 8 readable bytes after its end as for chgpu_string_dictionary_encode.  2^32 rows or more
   answer CHGPU_ERR_NOT_IMPLEMENTED.  Not included: collations, Nullable(String), FixedString, a sampled-threshold LIMIT path. */
int chgpu_string_sort_permutation(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, const chgpu_col * perm_in_u64,
                                  int descending, uint64_t limit, chgpu_col ** perm_out_u64);
/* ColumnString::permute / index (ColumnString.cpp, indexImpl): out[i] = value[indexes[i]], i < (limit ? min(limit, indexes.rows) :
   indexes.rows), as a new ColumnString: offsets rebuilt, every value followed by its zero byte.  Repeated indexes are allowed; indexes must
   be CHGPU_U64; an index >= rows answers CHGPU_ERR_BAD_ARGUMENTS (a device flag, never a fault), a value of 4 GiB or more
   CHGPU_ERR_NOT_IMPLEMENTED.  Offsets, types, NULL arguments, zero rows and the 8 readable bytes after chars: as above. */
int chgpu_string_index(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, const chgpu_col * indexes_u64,
                       uint64_t limit, chgpu_col ** out_offsets_u64, chgpu_col ** out_chars_u8);
/* ---- String predicates against a constant: a WHERE clause over a ColumnString -> a UInt8 column of 0/1, one byte per row (the mask
   chgpu_filter* / chgpu_and / chgpu_agg_add_block_filtered / chgpu_string_filter take).  Values, constants and patterns are binary-safe
   (zero bytes, bytes >= 0x80); `value` / `pattern` are host memory, no terminator, at most CHGPU_STR_CONST_MAX bytes -- a longer one
   answers CHGPU_ERR_NOT_IMPLEMENTED (the caller keeps its CPU function).  Offsets that break the ColumnString invariant answer
   CHGPU_ERR_BAD_ARGUMENTS; no rows give an empty column.  The kernels read values 8 bytes at a time (chars needs the same 8 readable
   bytes after its end as for chgpu_string_dictionary_encode).
   chgpu_string_cmp_const: equals .. greaterOrEquals (CHGPU_EQ .. CHGPU_GE) of FunctionsComparison.h, StringComparisonImpl::
     string_vector_constant -> memcmpSmallAllowOverflow15: the first min(len_a, len_b) bytes compared as UNSIGNED bytes, then the shorter
     string is the smaller one; lengths exclude the terminating zero.
   chgpu_string_match_const: kind CHGPU_STR_LIKE is like / notLike (MatchImpl over likePatternToRegexp: `%` any run of bytes, `_` exactly one
     character -- one UTF-8 sequence of 1-4 bytes by its lead byte, every continuation byte 10xxxxxx and inside the value, else no match at
     that position; newline is a character like any other; `\%` `\_` `\\` are the literal bytes, a backslash before any other byte is a literal
     backslash, a pattern ending in a lone backslash is CHGPU_ERR_BAD_ARGUMENTS); CHGPU_STR_CONTAINS is position(haystack, needle) != 0 (an
     occurrence lies wholly inside one value: it never touches the terminating zero or the next row); CHGPU_STR_STARTS_WITH /
     CHGPU_STR_ENDS_WITH are startsWith / endsWith.  The empty needle matches every row.  negate != 0 inverts the result (notLike, NOT ...). */
#define CHGPU_STR_CONST_MAX 256
enum { CHGPU_STR_LIKE = 0, CHGPU_STR_CONTAINS = 1, CHGPU_STR_STARTS_WITH = 2, CHGPU_STR_ENDS_WITH = 3 };
int chgpu_string_cmp_const(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int op,
                           const void * value, uint64_t value_bytes, chgpu_col ** out_u8);
int chgpu_string_match_const(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int kind,
                             const void * pattern, uint64_t pattern_bytes, int negate, chgpu_col ** out_u8);
/* What a LIKE pattern compiles to; host only, needs no context (both calls above choose their kernel by it).  A pattern whose only
   unescaped `%` stand at its ends and that has no unescaped `_` is one of the four literal routes -- `abc` equals, `abc%` startsWith,
   `%abc` endsWith, `%abc%` contains, `%` / `%%` contains the empty string (always true) -- with literal[literal_bytes] the unescaped bytes;
   anything else is CHGPU_STR_ROUTE_GENERAL.  tokens[n_tokens] is the pattern as the general matcher walks it, for every route: unescaped
   bytes, runs of `%` collapsed into one; bit (i & 31) of token_meta[i >> 5] says token i is a wildcard (`%` or `_`) and not a literal.
   n_percent / n_underscore count the unescaped `%` / `_` of the pattern as written.  A trailing lone backslash answers
   CHGPU_ERR_BAD_ARGUMENTS, more than CHGPU_STR_CONST_MAX pattern bytes CHGPU_ERR_NOT_IMPLEMENTED. */
enum { CHGPU_STR_ROUTE_EQUALS = 0, CHGPU_STR_ROUTE_STARTS_WITH = 1, CHGPU_STR_ROUTE_ENDS_WITH = 2, CHGPU_STR_ROUTE_CONTAINS = 3,
       CHGPU_STR_ROUTE_GENERAL = 4 };
typedef struct chgpu_like_plan
{
    int32_t route;          /* CHGPU_STR_ROUTE_* */
    uint32_t n_percent;
    uint32_t n_underscore;
    uint32_t literal_bytes; /* 0 for the general route */
    uint32_t n_tokens;
    uint32_t token_meta[CHGPU_STR_CONST_MAX / 32];
    uint8_t literal[CHGPU_STR_CONST_MAX];
    uint8_t tokens[CHGPU_STR_CONST_MAX];
} chgpu_like_plan;
int chgpu_like_compile(const void * pattern, uint64_t pattern_bytes, chgpu_like_plan * out);
/* ---- String functions: a new column computed from a ColumnString, on the device.  The conventions of the String calls above hold for
   all six: values are binary-safe (zero bytes and bytes >= 0x80 are ordinary bytes); lengths exclude the terminating zero; offsets that
   break the ColumnString invariant answer CHGPU_ERR_BAD_ARGUMENTS, as do NULL arguments and wrong column types; zero rows give empty
   columns; chars needs its 8 readable bytes after the end; a result ColumnString is an ordinary one (a zero after every value, cumulative
   offsets, out_chars.rows == offsets.back()); a value of 4 GiB or more answers CHGPU_ERR_NOT_IMPLEMENTED; a failed call frees what it
   allocated and leaves every *out untouched.  Every check that needs no device (NULL arguments, types, row counts, argument domains,
   constant sizes) is made before the first device call.
   chgpu_string_length (FunctionStringOrArrayToT over LengthImpl, LengthUTF8Impl, EmptyImpl): CHGPU_STR_LENGTH is length, the bytes, a
     UInt64 column; CHGPU_STR_LENGTH_UTF8 is lengthUTF8, the number of bytes b with (b & 0xC0) != 0x80 -- the reference's code-point count
     (UTF8::countCodePoints): every byte that is not a continuation byte, on valid and invalid UTF-8 alike -- a UInt64 column;
     CHGPU_STR_EMPTY and CHGPU_STR_NOT_EMPTY give a UInt8 0/1.
   chgpu_string_map_case (LowerUpperImpl): CHGPU_STR_LOWER is lower, CHGPU_STR_UPPER is upper, the ASCII forms: a byte in 'A'..'Z' (or
     'a'..'z') has bit 0x20 flipped, every other byte is copied.  The offsets are copied.  Bytes of a wrapped chars buffer behind
     offsets.back() are neither read into the result nor counted.  lowerUTF8 / upperUTF8 have no kind.
   chgpu_string_cmp_columns (StringComparisonImpl::string_vector_string_vector): CHGPU_EQ .. CHGPU_GE row by row, in the order of
     chgpu_string_cmp_const: unsigned bytes over the common prefix, then the shorter value is the smaller.  Different row counts answer
     CHGPU_ERR_SIZES_MISMATCH.  a and b may be the same column.
   chgpu_string_substring (FunctionsStringSubstring, SubstringImpl): substring(s, offset[, length]) with constant arguments, counted in
     bytes.  The result is the value's bytes inside a window: for offset >= 1 the window begins at byte index offset - 1; for
     offset <= -1 it begins at index size - |offset|, which may be negative; it covers `length` indexes (has_length != 0), or runs to the
     end of the value without a length; it is clipped to [0, size).  So substring('abc', -5, 3) = 'a', substring('abc', -5) = 'abc' and
     substring('abc', 4) = ''.  All arithmetic saturates: offset = INT64_MIN, offset - 1 + length past 2^64 and length = 2^64 - 1 are legal
     inputs.  offset == 0 answers CHGPU_ERR_NOT_IMPLEMENTED (the reference's answer there has changed between versions, so it is left
     out, not guessed).  A negative length, column arguments and substringUTF8 cannot be expressed.
   chgpu_string_concat (ConcatImpl): an argument is a column when offsets != NULL, otherwise a constant of value_bytes bytes in host memory.
     2 <= n_args <= 8 and at least one argument is a column, otherwise CHGPU_ERR_BAD_ARGUMENTS.  The constant bytes of one call together
     are at most CHGPU_STR_CONST_MAX, otherwise CHGPU_ERR_NOT_IMPLEMENTED (one kernel argument carries them: no upload per call).  All
     columns have the same row count, otherwise CHGPU_ERR_SIZES_MISMATCH.  The same column may appear several times.
   chgpu_string_position_const (PositionImpl::vectorConstant, the byte form): position(haystack, needle), the 1-based byte index of the
     first occurrence that lies wholly inside the value -- the rule of CHGPU_STR_CONTAINS: an occurrence never touches the terminating
     zero or the next row -- and 0 when there is none; a UInt64 column.  The empty needle gives 1 for every row.  A needle longer than
     CHGPU_STR_CONST_MAX answers CHGPU_ERR_NOT_IMPLEMENTED.  positionUTF8 and the case-insensitive forms have no entry point. */
enum { CHGPU_STR_LENGTH = 0, CHGPU_STR_LENGTH_UTF8 = 1, CHGPU_STR_EMPTY = 2, CHGPU_STR_NOT_EMPTY = 3 };
enum { CHGPU_STR_LOWER = 0, CHGPU_STR_UPPER = 1 };
typedef struct chgpu_string_arg
{
    const chgpu_col * offsets, * chars; /* a column; offsets == NULL: a constant */
    const void * value;                 /* the constant's bytes in host memory, no terminator */
    uint64_t value_bytes;
} chgpu_string_arg;
int chgpu_string_length(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int kind, chgpu_col ** out);
int chgpu_string_map_case(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int kind,
                          chgpu_col ** out_offsets_u64, chgpu_col ** out_chars_u8);
int chgpu_string_cmp_columns(chgpu_ctx * ctx, const chgpu_col * a_offsets_u64, const chgpu_col * a_chars_u8, const chgpu_col * b_offsets_u64,
                             const chgpu_col * b_chars_u8, int op, chgpu_col ** out_u8);
int chgpu_string_substring(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int64_t offset, int has_length,
                           uint64_t length, chgpu_col ** out_offsets_u64, chgpu_col ** out_chars_u8);
int chgpu_string_concat(chgpu_ctx * ctx, const chgpu_string_arg * args, uint32_t n_args, chgpu_col ** out_offsets_u64,
                        chgpu_col ** out_chars_u8);
int chgpu_string_position_const(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, const void * needle,
                                uint64_t needle_bytes, chgpu_col ** out_u64);
int chgpu_agg_create(chgpu_ctx * ctx, int key_type, uint32_t n_aggs, const int * agg_kinds, const int * arg_types,
                     uint64_t size_hint, chgpu_agg ** out);
/* executeOnBlock over rows [row_begin,row_end) of the key column and the argument columns (arg_cols[j] may be NULL
   for count()).  arg_cols is indexed by argument slot: see CHGPU_AGG_ARG_MIN for aggregates with two arguments. */
int chgpu_agg_add_block(chgpu_agg * agg, const chgpu_col * key_col, const chgpu_col * const * arg_cols,
                        uint64_t row_begin, uint64_t row_end);
/* The same over the rows of [row_begin,row_end) whose filter byte is non-zero -- a FilterTransform (FilterTransform.cpp:136-256)
   directly in front of the AggregatingTransform, fused: rows that fail the WHERE clause neither create groups nor update
   states.  Low-cardinality aggregations read the mask inside the aggregation kernel (no filtered copy of the columns is made);
   the other strategies filter the block's columns first (chgpu_filter_columns).  filter_u8 == NULL: plain add_block. */
int chgpu_agg_add_block_filtered(chgpu_agg * agg, const chgpu_col * key_col, const chgpu_col * const * arg_cols,
                                 uint64_t row_begin, uint64_t row_end, const chgpu_col * filter_u8);
/* mergeDataImpl: fold src's states into dst (src stays valid but should be freed) */
int chgpu_agg_merge(chgpu_agg * dst, const chgpu_agg * src);
/* merge partial states that arrive as columns (the ColumnAggregateFunction blocks of a distributed GROUP BY,
   Aggregator::mergeOnBlock :227): keys + one state column per aggregate (avg: two columns numerator, denominator
   passed consecutively in state_cols) */
int chgpu_agg_merge_states(chgpu_agg * dst, const chgpu_col * key_col, const chgpu_col * const * state_cols, uint64_t rows);
int chgpu_agg_size(chgpu_agg * agg, uint64_t * groups);
/* convertToBlockImplFinal: key column + one result column per aggregate (count -> U64, sum -> SumSimple type,
   avg -> F64).  Row order is table order (unspecified, as in the reference); keys_out may be NULL for without_key. */
int chgpu_agg_finalize(chgpu_agg * agg, chgpu_col ** keys_out, chgpu_col ** res_cols, uint64_t * groups);
/* convertToBlockImplNotFinal: raw states (sum/count 8 B; avg -> numerator, denominator as two columns) */
int chgpu_agg_export_states(chgpu_agg * agg, chgpu_col ** keys_out, chgpu_col ** state_cols, uint64_t * groups);
/* convertToBlockImplNotFinal for a two-level result (Aggregator::prepareBlocksAndFillTwoLevelImpl, Aggregator.cpp:2790-2860): the
   same states ordered by bucket = (crc32c(key) >> 24) & 0xFF (TwoLevelHashTable.h:53 getBucketFromHash over HashCRC32<Key>,
   Hash.h:280-288), bucket_counts[256] rows each -- bucket b is rows [sum(counts[:b]), +counts[b]): the 256 blocks with
   BlockInfo::bucket_num (src/Core/BlockInfo.h:21-29) a CPU initiator's MergingAggregatedMemoryEfficientTransform expects. */
int chgpu_agg_export_states_two_level(chgpu_agg * agg, chgpu_col ** keys_out, chgpu_col ** state_cols, uint64_t * groups,
                                      uint64_t * bucket_counts);
/* §8(f) rank 4 — partial states on the wire: the bytes IAggregateFunction::serialize writes for every row of a ColumnAggregateFunction
   (SerializationAggregateFunction: the rows' states one after the other, no lengths): sum = the 8-byte sum, little endian
   (AggregateFunctionSum.h:288-291); count = VarUInt (AggregateFunctionCount.h:126-129); avg = the 8-byte numerator + VarUInt denominator
   (AggregateFunctionAvg.h, AvgFraction).  word0 / word1 are the state columns chgpu_agg_export_states(_two_level) returns (word1: avg's
   denominator).  offsets_u64 (may be NULL) receives rows + 1 byte offsets, so the 256 bucket blocks of a two-level export can be cut
   out of one buffer.  deserialize is the inverse for mergeOnBlock: `n_streams` independent runs of states (stream s: stream_rows[s] states
   from byte stream_byte_begin[s]; a single stream may pass NULL) -> word columns for chgpu_agg_merge_states.  A state's length is only
   known after its VarUInt, so one lane walks one stream; bucket-wise exchanges give 256 streams per peer. */
int chgpu_agg_serialize_states(chgpu_ctx * ctx, int kind, const chgpu_col * word0, const chgpu_col * word1, chgpu_col ** bytes_u8, chgpu_col ** offsets_u64);
int chgpu_agg_deserialize_states(chgpu_ctx * ctx, int kind, const chgpu_col * bytes_u8, uint32_t n_streams, const uint64_t * stream_byte_begin,
                                 const uint64_t * stream_rows, chgpu_col ** word0, chgpu_col ** word1);
int chgpu_agg_free(chgpu_agg * agg);
/* ---- max_rows_to_group_by / group_by_overflow_mode / overflow_row (Aggregator::Params, src/QueryPipeline/SizeLimits.h OverflowMode) ----
   max_rows_to_group_by = 0: no limit (the default).  Set before the first block or merge, else CHGPU_ERR_BAD_ARGUMENTS; an unknown mode
   too.  Without key (key_type < 0) the limits are accepted and never trigger, and overflow_row has no effect.  With no limit and no
   overflow row, nothing changes. */
enum
{
    CHGPU_OVERFLOW_THROW = 0,
    CHGPU_OVERFLOW_BREAK = 1,
    CHGPU_OVERFLOW_ANY = 2
};
int chgpu_agg_set_limits(chgpu_agg * agg, uint64_t max_rows_to_group_by, int group_by_overflow_mode, int overflow_row);
/* executeOnBlock (Aggregator.cpp:1181-1194, :1611): filter_u8 may be NULL (as chgpu_agg_add_block_filtered).  *no_more_keys is the
   caller's, one per stream: when it is set every row FINDS its key and inserts none -- a row whose key the table lacks goes to the
   overflow row (overflow_row on) or is dropped.  Otherwise the block is added in full and checkLimits runs on the number of groups G
   (zero key included, overflow row excluded): G > max_rows_to_group_by -> THROW: CHGPU_ERR_TOO_MANY_ROWS ("Limit for rows to GROUP BY
   exceeded: has G rows, maximum: M"; the block stays added), BREAK: *keep_reading = 0 (not latched), ANY: *no_more_keys = 1. */
int chgpu_agg_execute_on_block(chgpu_agg * agg, const chgpu_col * key_col, const chgpu_col * const * arg_cols, uint64_t row_begin,
                               uint64_t row_end, const chgpu_col * filter_u8, int * no_more_keys, int * keep_reading);
/* One step of mergeSingleLevelDataImpl under limits (the caller merges the variants into the largest first, prepareVariantsToMerge):
   checkLimits on dst's size BEFORE src is merged, with the merge's own *no_more_keys -- THROW fails, BREAK: *keep_merging = 0 and only
   the overflow rows merge, ANY: find-only from here on (a source state whose key dst lacks goes to dst's overflow row, or is dropped
   without one).  Overflow rows always merge into dst's. */
int chgpu_agg_merge_limited(chgpu_agg * dst, const chgpu_agg * src, int * no_more_keys, int * keep_merging);
/* One mergeOnBlock under limits: find-only when *no_more_keys is set, checkLimits after the block (as executeOnBlock); a block flagged
   is_overflows (one row) merges into the overflow row. */
int chgpu_agg_merge_states_limited(chgpu_agg * dst, const chgpu_col * key_col, const chgpu_col * const * state_cols, uint64_t rows,
                                   int is_overflows, int * no_more_keys, int * keep_reading);
/* The overflow row (prepareBlockAndFillWithoutKey(..., is_overflows)): final != 0 -> one one-row result column per aggregate, else the
   raw state words (as chgpu_agg_export_states).  *has = 0 when there is none (no executeOnBlock yet with overflow_row on).  The
   overflow row is never part of chgpu_agg_size, the exports or chgpu_agg_finalize. */
int chgpu_agg_overflow_row(chgpu_agg * agg, int final, chgpu_col ** cols, int * has);
/* ---- the -If combinator and Nullable arguments (AggregateFunctionIf; AggregateFunctionNullUnary, AggregateFunctionCountNotNullUnary) ----
   Every aggregate function has a condition mode.  A group exists as soon as one of its rows passes the WHERE filter, whatever the
   per-function masks say (the key is emplaced before any add): masked-out rows count towards max_rows_to_group_by like any other.
     NONE  every row reaches the function.
     IF    a row reaches it when its UInt8 condition byte is non-zero (2 and 255 as much as 1).  No row reached it: count 0, sum 0,
           avg NaN, min / max / any / argMin / argMax the type's default.
     NULL  a row reaches it when its null-map byte is zero.  The result is Nullable: chgpu_agg_finalize_nullable returns the value
           column and a UInt8 null map; no row reached it: null-map byte 1 and the type's default as the nested value (avg: 0.0).
           count stays UInt64 without a map and counts the non-NULL rows.
   A two-argument function takes one condition column (the caller ORs the null maps); sumIf over a Nullable argument is NULL mode
   with the map `null OR NOT cond` (AggregateFunctionIfNullUnary).
   State words: a conditioned min / max and a NULL-mode sum carry one more public word behind their own, `seen` = the number of rows
   that reached the function (UInt64, merged by addition like a count); it travels through the exports and chgpu_agg_merge_states*
   like every other word.  More than 16 words in all: CHGPU_ERR_BAD_ARGUMENTS.  The wire bytes of chgpu_agg_serialize_states know
   nothing about it: an -If state serialises as its nested function's (count / sum / avg); NULL-mode states have no wire form here. */
enum { CHGPU_AGG_COND_NONE = 0, CHGPU_AGG_COND_IF = 1, CHGPU_AGG_COND_NULL = 2 };
/* before the first block or merge (else BAD_ARGUMENTS); cond_modes[n_aggs] */
int chgpu_agg_set_conditions(chgpu_agg * agg, const int * cond_modes);
/* cond_cols[n_aggs]: UInt8 columns over the same rows as the arguments (NULL where the mode is NONE); the same column may serve several
   functions.  filter_u8 (WHERE) may be NULL.  no_more_keys / keep_reading may both be NULL: then as chgpu_agg_add_block(_filtered),
   else as chgpu_agg_execute_on_block.  An aggregator without conditions accepts cond_cols == NULL; one WITH conditions only accepts
   this call (chgpu_agg_add_block, _filtered and chgpu_agg_execute_on_block answer BAD_ARGUMENTS). */
int chgpu_agg_execute_on_block_conditional(chgpu_agg * agg, const chgpu_col * key_col, const chgpu_col * const * arg_cols,
                                           const chgpu_col * const * cond_cols, uint64_t row_begin, uint64_t row_end,
                                           const chgpu_col * filter_u8, int * no_more_keys, int * keep_reading);
/* as chgpu_agg_finalize; null_maps[n_aggs] receives a UInt8 column for every NULL-mode function but count, NULL elsewhere.
   (chgpu_agg_finalize itself applies the defaults too, and answers BAD_ARGUMENTS when a map would be lost.) */
int chgpu_agg_finalize_nullable(chgpu_agg * agg, chgpu_col ** keys_out, chgpu_col ** res_cols, chgpu_col ** null_maps, uint64_t * groups);

/* ================================================================================================
 * a19/a20 hash join  —  IJoin::addBlockToJoin / onBuildPhaseFinish / joinBlock (src/Interpreters/IJoin.h:80-93,142)
 * for HashJoin key64 (one numeric key up to 8 bytes; src/Interpreters/HashJoin/HashJoin.cpp:254-356,556-768,1036-1101;
 * HashJoinMethodsImpl.h:220-281,402-549).  RowRef{block*,row} becomes a global build row id
 * (block_index << 32 | row_in_block); RowRefList's linked 7-slot batches become one CSR array.
 * ============================================================================================== */
int chgpu_join_create(chgpu_ctx * ctx, int key_type, int kind, int strictness, int any_take_last_row,
                      uint64_t size_hint, chgpu_join ** out);
/* null_map_u8 / join_mask_u8 may be NULL (rows with null key or failed ON mask are not inserted, Impl.h:261-272).
   block_index_out receives the index the block got (0,1,2...).  rows >= 2^32 -> CHGPU_ERR_TOO_MANY_ROWS. */
int chgpu_join_add_block(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * null_map_u8,
                         const chgpu_col * join_mask_u8, uint32_t * block_index_out);
/* IJoin::onBuildPhaseFinish: no more right blocks.  The hash table is built lazily, by the first call that needs it (chgpu_join_probe, the key
   count of chgpu_join_total_rows, chgpu_join_non_joined_rows); chgpu_join_probe_agg over a large unique-key build side joins without one. */
int chgpu_join_finish_build(chgpu_join * j);
int chgpu_join_total_rows(chgpu_join * j, uint64_t * rows, uint64_t * keys);
/* joinRightColumns over the left key column.  Outputs (all device columns, caller frees; unused ones are NULL):
     filter_u8        [n_left_consumed]  need_filter variants (INNER ANY, LEFT SEMI, LEFT ANTI)
     offsets_u64      [n_left_consumed]  need_replication variants (ALL): cumulative offsets_to_replicate
     right_rowid_u64  [n_out]            one entry per appended right row: (block<<32|row), all-ones = default row;
                                         may be NULL for LEFT SEMI / LEFT ANTI when the right side contributes no columns
                                         (an empty AddedColumns, AddedColumns.h): only the filter and n_out are produced
   max_joined_block_rows: 0 = unlimited; else processing stops BEFORE the first left row at which the running
   output count is already >= max (HashJoinMethodsImpl.h:436-444) and n_left_consumed < rows tells the caller to
   resubmit the tail (JoiningTransform.cpp:220-260). */
int chgpu_join_probe(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * null_map_u8,
                     uint64_t max_joined_block_rows, chgpu_col ** filter_u8, chgpu_col ** offsets_u64,
                     chgpu_col ** right_rowid_u64, uint64_t * n_out, uint64_t * n_left_consumed);
/* joinBlock with the aggregation that consumes its output fused behind it: `SELECT count(), sum(right.payload) FROM left JOIN right`
   (HashJoinMethodsImpl.h:402-549 -> AddedColumns' lazy gather, AddedColumns.cpp:39-131 -> Aggregator::executeWithoutKeyImpl,
   Aggregator.cpp:1276-1321).  One pass over the left keys; nothing per left row is written (no offsets_to_replicate, no row ids, no
   gathered column).  *count_out = rows the join would emit; sum_out = 8 bytes typed like SumSimple(payload type): the sum of the
   payload over those rows (default rows of LEFT joins add 0; LEFT ANTI emits no right row).  right_payload is the right Blocks'
   column glued in insertion order (chgpu_col_concat), may be NULL for count only.  Variants: INNER ALL, LEFT ALL, LEFT ANY,
   LEFT SEMI, LEFT ANTI; INNER ANY / RIGHT / FULL -> CHGPU_ERR_NOT_IMPLEMENTED (stateful across calls: use chgpu_join_probe).
   Float sums are reduced in a fixed order: run-to-run reproducible. */
int chgpu_join_probe_agg(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * null_map_u8, const chgpu_col * right_payload,
                         uint64_t * count_out, void * sum_out);
/* A CHAIN of JoiningTransforms answered in one sweep over the left key columns (late materialisation).  When every join of the chain is of
   the filter form -- LEFT SEMI, LEFT ANTI, or ALL over a build side without duplicate keys: HashJoinMethodsImpl.h:68-202 then computes a
   filter and calls `block.filter(filter)` (:122-123) on EVERY left column, once per join -- the left rows that survive the whole chain are
   the AND of the joins' filters and no join changes a row's multiplicity.  This entry computes that AND before any left column is copied
   (key_cols[s] is probed against joins[s]; null_maps / null_maps[s] may be NULL): dense dimension key sets are staged in LDS, the other
   steps are probed only for the rows still alive.  Outputs, all sized by the survivors (*n_kept) and in ascending left-row order; every
   output pointer may be NULL when not wanted:
     indexes_u64          the surviving left row numbers (filterToIndices, src/Columns/FilterDescription.cpp:113-116)
     right_rowid_u64[s]   for steps with want_right_rows[s] != 0: the matched build row (block << 32 | row) of joins[s], all-ones where the
                          join adds a default row (LEFT joins without a match, ANTI) -- what chgpu_join_probe would return over the survivors
     carry_out[c]         carry_cols[c] gathered at the survivors (IColumn::index; the chain's `block.filter` over the left columns)
     filter_u8 [rows]     the chain's IColumn::Filter itself, 1 = the row survives every join
   LEFT ANY / LEFT ALL steps keep every left row (they only contribute right_rowid).  INNER ANY, RIGHT, FULL (stateful across calls) and ALL
   over duplicate build keys (replicates rows) -> CHGPU_ERR_NOT_IMPLEMENTED: run those joins one by one with chgpu_join_probe. */
int chgpu_join_probe_chain(uint32_t n_steps, chgpu_join * const * joins, const chgpu_col * const * key_cols, const chgpu_col * const * null_maps,
                           const int * want_right_rows, uint32_t n_carry, const chgpu_col * const * carry_cols, chgpu_col ** indexes_u64,
                           chgpu_col ** right_rowid_u64, chgpu_col ** carry_out, chgpu_col ** filter_u8, uint64_t * n_kept);
/* The same with ONE right column per payload step gathered inside the call (AddedColumns' lazy columns, AddedColumns.cpp:39-131): right_cols[s]
   != NULL (a step with want_right_rows[s], over a one-block build side) makes right_out[s] that column's values at the matched rows -- a miss
   gives the type's default -- instead of the row ids; steps with right_cols[s] == NULL still return row ids in right_out[s]. */
int chgpu_join_probe_chain_columns(uint32_t n_steps, chgpu_join * const * joins, const chgpu_col * const * key_cols, const chgpu_col * const * null_maps,
                                   const int * want_right_rows, const chgpu_col * const * right_cols, uint32_t n_carry, const chgpu_col * const * carry_cols,
                                   chgpu_col ** indexes_u64, chgpu_col ** right_out, chgpu_col ** carry_out, chgpu_col ** filter_u8, uint64_t * n_kept);
/* (block_index << 32 | row) ids -> running ordinal of the row over all right blocks in insertion order (all-ones stays
   all-ones): the index into payload columns concatenated with chgpu_col_concat, i.e. fillFromBlocksAndRowNumbers
   (src/Columns/IColumn.cpp:515-526) for many right Blocks */
int chgpu_join_flatten_rowids(chgpu_join * j, const chgpu_col * right_rowid_u64, chgpu_col ** flat_u64);
/* IJoin::getNonJoinedBlocks (src/Interpreters/IJoin.h:133-134; NotJoinedHash, HashJoin.cpp:1280-1420) for RIGHT / FULL joins (strictness
   ALL): every right row a joinBlock emitted is flagged (JoinUsedFlags); after the last joinBlock this returns the build rows no left row
   matched -- rows with a NULL key or a zero ON mask included -- as (block << 32 | row) ids in insertion order.  RIGHT probes like INNER,
   FULL like LEFT. */
int chgpu_join_non_joined_rows(chgpu_join * j, chgpu_col ** right_rowid_u64, uint64_t * rows_out);
int chgpu_join_free(chgpu_join * j);

/* ================================================================================================
 * (e) multi-GPU  —  the exchange step of the sharded operators over RCCL (xGMI inside a node); one process per GPU.
 * ConcurrentHashJoin::dispatchBlock hands the sub-blocks of a scattered Block to the per-slot HashJoins
 * (src/Interpreters/ConcurrentHashJoin.cpp:538-565), a parallel merge hands two-level buckets to their owners
 * (ConcurrentHashJoin.cpp:600-653; src/Processors/Transforms/AggregatingTransform.cpp:120-136): threads of one address space there,
 * ranks exchanging hash partitions here.  Shard of a key = ((crc32c(key) >> 24) & 0xFF) & (world - 1) (chgpu_hash_to_selector),
 * so world is a power of two <= 256 (ConcurrentHashJoin.cpp:158).  A communicator binds one rank to one chgpu_ctx; all its
 * traffic runs on that context's stream.  librccl is loaded on first use; without it these calls fail with CHGPU_ERR_DEVICE.
 * Sequence: rank 0 calls chgpu_comm_unique_id and hands the 128 bytes to every rank out of band (the host pipeline's own control
 * plane), every rank calls chgpu_comm_init (collective).  Then per exchange: chgpu_partition_by_hash -> chgpu_all_to_all_counts
 * -> chgpu_all_to_all per column.
 * ============================================================================================== */
#define CHGPU_UNIQUE_ID_BYTES 128
typedef struct chgpu_comm chgpu_comm;
int chgpu_comm_unique_id(uint8_t id_out[CHGPU_UNIQUE_ID_BYTES]);
int chgpu_comm_init(chgpu_ctx * ctx, int rank, int world, const uint8_t unique_id[CHGPU_UNIQUE_ID_BYTES], chgpu_comm ** out);
int chgpu_comm_destroy(chgpu_comm * comm);
int chgpu_comm_rank(const chgpu_comm * comm);
int chgpu_comm_world(const chgpu_comm * comm);
/* [0] bytes sent to other ranks [1] bytes received from other ranks [2] collectives issued */
int chgpu_comm_stats(const chgpu_comm * comm, uint64_t out[3]);
/* recv_counts[p] = the send_counts[my rank] of rank p: sizes the receive side of the all-to-all that follows (host arrays of `world`) */
int chgpu_all_to_all_counts(chgpu_comm * comm, const uint64_t * send_counts, uint64_t * recv_counts);
/* send: shards back to back as chgpu_partition_by_hash returns them (shard p = send_counts[p] rows for rank p); *recv_out: a new column of
   sum(recv_counts) rows, what ranks 0..world-1 sent here in rank order.  One grouped send/recv: every xGMI link carries its peer's
   partition at once; the own partition is a device copy.  Asynchronous on the context's stream. */
int chgpu_all_to_all(chgpu_comm * comm, const chgpu_col * send, const uint64_t * send_counts, const uint64_t * recv_counts, chgpu_col ** recv_out);
/* The exchange of a whole Block: n_cols columns that share their partition boundaries (chgpu_partition_by_hash's outputs: the key column
   and every state / payload column) leave in ONE grouped send / recv over all columns and peers, after ONE exchange of the row counts
   (recv_counts [world] is an output: the rows each rank sent here).  What dispatchBlock + the shard's input port do for one Block
   (src/Interpreters/ConcurrentHashJoin.cpp:538-565).  chgpu_all_to_all_counts + chgpu_all_to_all remain for a single column. */
int chgpu_all_to_all_multi(chgpu_comm * comm, uint32_t n_cols, const chgpu_col * const * send, const uint64_t * send_counts, uint64_t * recv_counts,
                           chgpu_col ** recv_out);
/* mergeWithoutKeyDataImpl across ranks (src/Interpreters/Aggregator.cpp:2584-2628): element-wise wrap-around sum of a UInt64 / Int64
   device column over all ranks, in place (asynchronous); _host: the same for <= 64 host values (synchronises) */
int chgpu_all_reduce_u64(chgpu_comm * comm, chgpu_col * inout_u64);
int chgpu_all_reduce_u64_host(chgpu_comm * comm, uint64_t * values, uint32_t n);
/* returns once every rank's queued work on its stream has finished */
int chgpu_comm_barrier(chgpu_comm * comm);

#ifdef __cplusplus
}
#endif
#endif /* CHGPU_H */
