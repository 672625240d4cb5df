/*
 * include/gossip/gossip.h -- the drop-in boundary of the MI355X gossip-membership engine.
 *
 * Plain C ABI (extern "C", plain pointers and sizes, int status returns, no exceptions
 * and no torch/HIP types) over libgossip_amd.so.  Two engines live behind it:
 *
 *  gsp_engine  -- EXACT mode: the reference MP1 semantics, bit-exact.  The caller drives
 *                 it with the same per-tick call pattern the reference Application uses
 *                 on MP1Node/EmulNet (/root/reference/Application.cpp:121-202); the
 *                 engine batches the calls of one phase and runs them as HIP kernels
 *                 (merge = MP1Node::recvCallBack, ops = MP1Node::nodeLoopOps).  The C++
 *                 facade in <gossip/mp1_facade.hpp> keeps the reference's class and method
 *                 names on top of these entry points.
 *  gsp_scale   -- SCALE mode: the build-defined full-view protocol with the
 *                 membership table resident in HBM as packed 16-bit entries and one fused
 *                 HIP kernel per tick; rows sharded over GPUs.
 *
 * Every entry point returns GSP_OK (0) or a negative gsp_status.  gsp_last_error()
 * returns a human-readable message for the last failure on the calling thread.
 * Threading: an engine is used by one host thread at a time.  Ownership: the engine
 * owns all device and pinned memory; callers own every buffer they pass in.
 */
#ifndef GOSSIP_GOSSIP_H
#define GOSSIP_GOSSIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSP_ABI_VERSION 7

typedef enum {
    GSP_OK = 0,
    GSP_ERR_INVALID = -1,      /* bad argument                                       */
    GSP_ERR_IO = -2,           /* file could not be read / written                   */
    GSP_ERR_HIP = -3,          /* a HIP runtime call failed (no GPU, OOM, fault)      */
    GSP_ERR_ORDER = -4,        /* call order the batched engine cannot reproduce     */
    GSP_ERR_CAPACITY = -5,     /* a device buffer bound was exceeded                  */
    GSP_ERR_RCCL = -6,         /* an RCCL call failed                                  */
    GSP_ERR_RANGE = -7         /* a value would overflow its packed representation   */
} gsp_status;

const char *gsp_last_error(void);
int gsp_abi_version(void);
/* Number of visible HIP devices (0 when none); never fails. */
int gsp_device_count(void);

/* ------------------------------------------------------------------------------------
 * Replay draws.  The counter-based Philox4x32-10 the engine uses in GSP_RNG_PHILOX mode,
 * host-callable so that the reference-side EmulNet replay hook can make
 * the identical draw in place of rand() at EmulNet.cpp:89 and Application.cpp:182/189:
 *   drop draw:  gsp_replay_draw(GSP_DOMAIN_SEND, seed, tick, src_id, dst_id, msgType)
 *   fail draw:  gsp_replay_draw(GSP_DOMAIN_FAIL, seed, tick, 0, 0, 0)
 * The value is in [0, 2^31) like rand().
 * ---------------------------------------------------------------------------------- */
#define GSP_DOMAIN_SEND 0x53454E44u
#define GSP_DOMAIN_FAIL 0x4641494Cu
#define GSP_DOMAIN_PEER 0x50454552u
#define GSP_DOMAIN_PING 0x50494E47u
#define GSP_DOMAIN_JOIN 0x4A4F494Eu
uint32_t gsp_replay_draw(uint32_t domain, uint64_t seed, uint32_t a, uint32_t b, uint32_t c,
                         uint32_t d);
int gsp_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* ------------------------------------------------------------------------------------
 * Params -- /root/reference/Params.{h,cpp}.  gsp_params_from_conf parses the same
 * four-key .conf grammar as Params::setparams (Params.cpp:19-43) and fills the same
 * hard-coded values (STEP_RATE 0.25, MAX_MSG_SIZE 4000, Params.cpp:29-31).
 *
 * The box gsp_create admits (anything outside: GSP_ERR_INVALID naming the field, before any
 * HIP call):
 *   max_nnb             1 .. 1024
 *   msg_drop_prob       0 .. 1, finite (the threshold is (int)(100 p), EmulNet.cpp:92)
 *   step_rate           >= 0, finite (0: every node starts at tick 0)
 *   max_msg_size        >= 0 (every send is 40 + 16 bytes: <= 56 rejects all, >= 57 none)
 *   en_buff_size        0 .. 2^20 - 1 (a node's queue index has 20 bits in the list order key)
 *   total_running_time  1 .. 3600 (MAX_TIME, EmulNet.h:11)
 *   tremove             >= 1
 *   id_filter_limit     >= 0 (> max_nnb: no payload entry is filtered)
 *   intro_list          0 .. 16
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t max_nnb;            /* MAX_NNB -> EN_GPSZ, the number of peers             */
    int32_t single_failure;     /* SINGLE_FAILURE                                      */
    int32_t drop_msg;           /* DROP_MSG                                            */
    double msg_drop_prob;       /* MSG_DROP_PROB                                       */
    double step_rate;           /* STEP_RATE (join schedule), 0.25                      */
    int32_t max_msg_size;       /* MAX_MSG_SIZE, 4000                                  */
    int32_t en_buff_size;       /* EmulNet buffer bound, ENBUFFSIZE 30000 (EmulNet.h:12) */
    int32_t total_running_time; /* TOTAL_RUNNING_TIME, 700 (Application.h:27)          */
    int32_t tremove;            /* TREMOVE, 20 (MP1Node.h:21)                          */
    int32_t id_filter_limit;    /* payload filter id < limit, 10 (MP1Node.cpp:245)     */
    int32_t intro_list;         /* opt-in protocol variant, 0 = the reference: the JOINREP
                                   carries the introducer's whole list and its receiver ignores
                                   it (MP1Node.cpp:221-233).  B = 1..16: the joiner merges B
                                   entries of the introducer's list, chosen by sequential
                                   distinct Philox ranks over list order (Philox(JOIN; t - 1,
                                   0, joiner index, i), t = the handling tick), with the GOSSIP
                                   payload rules (MP1Node.cpp:244-258, id filter included); the
                                   list is the introducer's as of the end of the tick it
                                   replied (the snapshot its GOSSIPs of that tick carry)      */
} gsp_params;

int gsp_params_default(gsp_params *out);
int gsp_params_from_conf(const char *path, gsp_params *out);

/* ------------------------------------------------------------------------------------
 * EXACT engine
 * ---------------------------------------------------------------------------------- */
typedef struct gsp_engine gsp_engine;

typedef enum {
    GSP_RNG_GLIBC = 0,  /* the reference's srand(seed)/rand() stream, indexed by draw order */
    GSP_RNG_PHILOX = 1  /* counter-based replay: Philox4x32-10(seed; tick, src, dst, type)  */
} gsp_rng_mode;

typedef enum {          /* message types, /root/reference/MP1Node.h:31-36 */
    GSP_MSG_JOINREQ = 0,
    GSP_MSG_JOINREP = 1,
    GSP_MSG_GOSSIP = 3
} gsp_msg_type;

typedef enum {          /* per-node operations of one phase-P batch */
    GSP_OP_START = 0,   /* MP1Node::nodeStart     (MP1Node.cpp:67)                     */
    GSP_OP_LOOP = 1,    /* MP1Node::nodeLoop      (MP1Node.cpp:176): drain + ops if inGroup */
    GSP_OP_CHECK = 2,   /* MP1Node::checkMessages (MP1Node.cpp:200): drain only         */
    GSP_OP_OPS = 3      /* MP1Node::nodeLoopOps   (MP1Node.cpp:335)                      */
} gsp_op;

/* Create an engine for p->max_nnb nodes (<= 1024) on HIP device `device`.
 * dbg_log_path: where the dbg.log event stream is written (NULL: keep in memory only).
 * The engine assigns node i the address id i+1, port 0 (EmulNet::ENinit, EmulNet.cpp:72). */
int gsp_create(const gsp_params *p, int device, gsp_rng_mode rng, uint64_t seed,
               const char *dbg_log_path, gsp_engine **out);
int gsp_destroy(gsp_engine *e);

/* Phase R: EmulNet::ENrecv for each node in `order`, in that order (the reference calls
 * MP1Node::recvLoop for i ascending, Application.cpp:125-135).  Delivery follows the
 * reference buffer permutation (top-down scan, swap-with-last, EmulNet.cpp:151-161). */
int gsp_tick_recv(gsp_engine *e, int32_t tick, const int32_t *order, int32_t n);

/* Phase P: one batch of per-node operations, executed in `order` (the reference calls
 * them for i descending, Application.cpp:138-163).  dropmsg is Params::dropmsg at call
 * time.  A node may appear at most once per batch. */
int gsp_tick_process(gsp_engine *e, int32_t tick, const int32_t *order, const int8_t *ops,
                     int32_t n, int32_t dropmsg);

/* EmulNet::ENsend issued directly by the caller (EmulNet.cpp:87-118): one draw, the drop
 * window and buffer bound, then the message joins the buffer.  A GOSSIP's payload is the
 * sender's current member list.  Returns GSP_OK; *admitted = message size or 0. */
int gsp_send(gsp_engine *e, int32_t tick, int32_t src_node, int32_t dst_id, int32_t type,
             int32_t dropmsg, int32_t *admitted);

/* One rand() draw in the engine's global draw order (the draw Application::fail makes,
 * Application.cpp:182/189).  In Philox mode the draw is Philox(seed; tick, 0, 0, 0). */
int gsp_rand(gsp_engine *e, int32_t tick, int32_t *value);

/* srand(seed) (Application.cpp:50/96): the next draw is the first of seed's stream (glibc
 * mode: the TYPE_3 stream of srand(seed) restarts at that draw; Philox mode: seed becomes
 * the replay key).  Draws already made are not affected. */
int gsp_srand(gsp_engine *e, uint64_t seed);

/* A line from the driver into dbg.log, ordered after all work submitted before it
 * (Log::LOG, Log.cpp:44).  node < 0 prints the empty address of the very first LOG. */
int gsp_log(gsp_engine *e, int32_t node, int32_t tick, const char *text);

/* Member mirror (/root/reference/Member.h:89-122). */
typedef struct {
    int32_t id;
    int16_t port;
    int8_t inited, in_group, failed;
    int64_t heartbeat;
    int32_t n_members;
} gsp_member_view;
typedef struct {
    int32_t id;
    int16_t port;
    int64_t heartbeat;
    int64_t timestamp;
} gsp_entry;
int gsp_set_failed(gsp_engine *e, int32_t node, int32_t failed);
int gsp_get_member(gsp_engine *e, int32_t node, gsp_member_view *out);
/* The member list of `node` in list order (MemberListEntry vector order). */
int gsp_member_list(gsp_engine *e, int32_t node, gsp_entry *buf, int32_t cap, int32_t *n);
/* The member lists of n nodes with one device read: list i (list order) at buf + i * N,
 * N = max_nnb entries each, its length in lens[i]. */
int gsp_member_lists(gsp_engine *e, const int32_t *nodes, int32_t n, gsp_entry *buf,
                     int32_t *lens);

/* MP1Node::addMember on `node`'s committed list at `tick` (MP1Node.cpp:265-301), a list
 * change of its own (the list's send-time version changes as after a batch):
 *  GSP_ADD_SENDER  addMember(MessageHdr *): entry->id absent -> appended as (id, 1, tick)
 *                  with its "joined" dbg.log line; present -> nothing;
 *  GSP_ADD_COPY    addMember(MemberListEntry *): the node itself -> nothing; else, when
 *                  tick - entry->timestamp < TREMOVE, the entry is appended as given with its
 *                  "joined" line.  The reference appends without looking the id up (its
 *                  callers check_exist first); an id already listed is GSP_ERR_INVALID here,
 *                  since a list holds each id once.
 * entry: id 1..N, port 0 (heartbeat / timestamp within int32).  *added = 1 if appended. */
#define GSP_ADD_SENDER 0
#define GSP_ADD_COPY 1
int gsp_add_member(gsp_engine *e, int32_t tick, int32_t node, const gsp_entry *entry,
                   int32_t mode, int32_t *added);

/* gsp_send with the message's own list (MessageHdr::vector_list of a message the driver
 * built, MP1Node.cpp:355-359): `payload` holds n_payload entries (ids 1..N, port 0, each id
 * once), which the receiver merges instead of the sender's committed list.  payload NULL is
 * gsp_send. */
int gsp_send_list(gsp_engine *e, int32_t tick, int32_t src_node, int32_t dst_id, int32_t type,
                  int32_t dropmsg, const gsp_entry *payload, int32_t n_payload, int32_t *admitted);

/* ---- Driver-side receive: EmulNet::ENrecv with the driver's own callback and direct
 * MP1Node::recvCallBack calls (MP1Node.cpp:46, 209, 219).  The reference hands the callback
 * each message as a MessageHdr whose vector_list is the sender's list at send time
 * (MP1Node.cpp:138/227/357); these calls move such messages between the engine and the
 * driver with that list attached, so a driver can observe, drop, reorder, hold back or
 * rewrite messages and process them one at a time.  mp1_facade.hpp builds the reference's
 * ENrecv / recvCallBack / checkMessages on them. */
typedef struct {
    int32_t src_id;       /* the sender's address id (MessageHdr::addr)                    */
    int32_t type;         /* gsp_msg_type (MessageHdr::msgType)                            */
    int64_t send_batch;   /* engine-side payload version (opaque to the driver)            */
    int64_t payload_off;  /* gsp_recv_detach: first entry of the payload in `payload`      */
    int32_t payload_len;  /* payload entries (MessageHdr::vector_list.size())              */
    int32_t pad;
} gsp_queued_msg;

/* Keep each sender's send-time list while messages carry it and the sender commits a newer
 * one.  Off by default below max_nnb = 512: a driver that runs each phase as one batch does not
 * need it while every id has an address class of its own.  On from gsp_create at max_nnb >= 512,
 * where ids 256 and 512 (then 768, 1024) compare equal under strcmp() (EmulNet.cpp:154) and one
 * of them takes, ticks later, the messages that lingered for the other.  Needed
 * once messages can be handled in separate batches (driver callbacks, gsp_recv_callback,
 * gsp_add_member), so mp1_facade.hpp turns it on when its EmulNet is constructed: every
 * message admitted from then on holds its list, whatever receive path the driver takes
 * later. */
int gsp_payload_snapshots(gsp_engine *e, int32_t on);

/* EmulNet::ENrecv for `node` with a driver callback (EmulNet.cpp:151-173): takes the node's
 * messages off the EmulNet buffer in the reference's delivery order, counts them as received
 * at `tick` (msgcount.log), and returns them with their payloads instead of queueing them.
 * msgs == NULL: sizes only (*n messages, *n_payload entries), nothing taken.  A buffer too
 * small for the sizes is GSP_ERR_CAPACITY with nothing taken. */
int gsp_recv_detach(gsp_engine *e, int32_t tick, int32_t node, gsp_queued_msg *msgs, int32_t cap,
                    gsp_entry *payload, int64_t payload_cap, int32_t *n, int64_t *n_payload);

/* Queue::enqueue into `node`'s queue (Queue.h:22-26), processed by the node's next
 * checkMessages / nodeLoop in queue order.  payload: m->payload_len entries, ids 1..N with
 * port 0, each id once (the list the message carries); NULL: the payload is the sender's list
 * of version m->send_batch, which the engine must still hold (GSP_ERR_ORDER otherwise). */
int gsp_queue_push(gsp_engine *e, int32_t node, const gsp_queued_msg *m, const gsp_entry *payload);

/* MP1Node::recvCallBack(env, data, size) called directly (MP1Node.cpp:219-260): `node`
 * processes exactly this message now -- the merge, a JOINREP reply with its draw -- and its
 * queue is left as it was.  payload as for gsp_queue_push. */
int gsp_recv_callback(gsp_engine *e, int32_t tick, int32_t node, const gsp_queued_msg *m,
                      const gsp_entry *payload, int32_t dropmsg);

/* Every node's end-of-tick state appended to `path`, one line per node in id order:
 * "t id inited inGroup bFailed heartbeat |L| id:hb:ts ..." with the list in MemberListEntry
 * order (Member.h:89-122) -- the state format of the parity fixtures.  bFailed is the flag set
 * by gsp_set_failed (Application::fail, Application.cpp:186/194). */
int gsp_state_dump(gsp_engine *e, int32_t tick, const char *path);

/* EmulNet::ENcleanup (EmulNet.cpp:184-220): writes msgcount.log for ticks [0, tick). */
int gsp_write_msgcount(gsp_engine *e, const char *path, int32_t tick);
/* Per-(node, tick) counters: sent[(id) * ticks + t], recv likewise, id in 1..N. */
int gsp_counters(gsp_engine *e, int32_t *sent, int32_t *recv, int32_t ticks);
/* Flush buffered dbg.log bytes to disk (done automatically on destroy). */
int gsp_flush_log(gsp_engine *e);
/* Copy the whole dbg.log byte stream produced so far. *n receives the full size. */
int gsp_log_bytes(gsp_engine *e, char *buf, size_t cap, size_t *n);

typedef struct {
    int64_t batches;            /* phase-P batches executed on the device             */
    int64_t node_rounds;        /* GSP_OP_LOOP operations executed                      */
    int64_t merges;             /* member-entry merges: 1 + |payload| per GOSSIP        */
    int64_t draws;              /* rand() draws consumed                                */
    int64_t sends_admitted;     /* messages appended to the EmulNet buffer             */
    double device_ms;           /* time inside the exact-mode kernels (HIP events)     */
} gsp_exact_stats;
int gsp_exact_stats_get(gsp_engine *e, gsp_exact_stats *out);

/* ------------------------------------------------------------------------------------
 * Driver policies of the scale engines.  The reference hard-codes them in
 * its driver -- node i starts at tick (int)(STEP_RATE * i) (Application.cpp:143,
 * Params.cpp:30), messages are dropped from the end of t = 50 to the end of t = 300, i.e.
 * the sends of ticks [51, 301) (Application.cpp:177, 198: fail() sets and clears the flag
 * after that tick's mp1Run), one random node or N/2 contiguous nodes crash at t = 100 (Application.cpp:180-196);
 * the scale engines take them as data, run on the device.  All zeros = the pre-joined,
 * always-dropping, single-event protocol of ABI 2.
 * ---------------------------------------------------------------------------------- */
#define GSP_MAX_FAIL_EVENTS 8
typedef enum {
    GSP_FAIL_NONE = 0,
    GSP_FAIL_RANDOM = 1,   /* each node with probability ppm / 10^6                        */
    GSP_FAIL_BLOCK = 2,    /* n * ppm / 10^6 contiguous nodes from a Philox start (wrapping) */
    GSP_FAIL_SINGLE = 3,   /* one node: Philox % n (Application.cpp:182)                    */
    GSP_FAIL_HALF = 4      /* n / 2 contiguous nodes from (Philox % n) / 2 (Application.cpp:189) */
} gsp_fail_mode;
typedef struct {
    int32_t tick;          /* the nodes crash at the end of this tick                       */
    int32_t mode;          /* gsp_fail_mode                                                 */
    int32_t ppm;           /* fraction for RANDOM / BLOCK, parts per million                */
} gsp_fail_event;
typedef struct {
    int32_t drop_from, drop_until;  /* drop_pct applies to the sends of ticks t with
                                       drop_from <= t < drop_until (drop_until <= 0: no end) */
    double step_rate;               /* join schedule: node i starts at tick (int)(step_rate * i);
                                       0: every node pre-joined.  Nodes starting at 0 list each
                                       other; a later node starts with an empty list and, one
                                       tick before, node 0 (the introducer, MP1Node.cpp:378-386)
                                       sends it a JOINREP if alive (drop draw Philox(SEND; t, 0,
                                       j, JOINREP)).  The JOINREP merges like a GOSSIP from node
                                       0 whose payload is the bounded introducer list below.   */
    int32_t intro_list;             /* JOINREP payload bound B (0..16): B members of node 0's
                                       gossipable list, Philox-chosen (Philox(JOIN; t, 0, j, i)
                                       sequential distinct ranks) -- MP1Node.cpp:221-230 sends
                                       the whole list and its receiver ignores it (:231-233)   */
    int32_t n_fail_events;          /* further crash events, applied after the one of
                                       (fail_mode, fail_tick, fail_ppm); event e draws with
                                       index e + 1                                           */
    gsp_fail_event fail_events[GSP_MAX_FAIL_EVENTS];
} gsp_policy;

/* The crash tick of every node under a failure schedule -- the first event (mode, tick, ppm of
 * gsp_scale_params / gsp_pview_params) and policy's further events, with the engines' own
 * Philox draws; INT32_MAX = never.  Host only (no device needed): lets a driver know which
 * nodes crashed, e.g. to measure failure detection from the event stream.  pol may be NULL. */
int gsp_fail_schedule(const gsp_policy *pol, int32_t n, uint64_t seed, int32_t mode, int32_t tick,
                      int32_t ppm, int32_t *out);

/* ------------------------------------------------------------------------------------
 * SCALE engine (full view, packed entries, device-resident tick loop)
 * ---------------------------------------------------------------------------------- */
typedef struct gsp_scale gsp_scale;

typedef struct {
    int32_t n;          /* nodes; full view V = n                                     */
    int32_t fanout;     /* peers per sender per tick (distinct), 1..16                 */
    int32_t drop_pct;   /* a send is dropped iff Philox % 100 < drop_pct               */
    int32_t tremove;    /* TREMOVE (20)                                                */
    int32_t h0;         /* initial heartbeat of every pre-joined entry (>= 1)          */
    int32_t fail_mode;  /* 0 none, 1 per-node Bernoulli(fail_ppm), 2 contiguous block  */
    int32_t fail_tick;  /* failed nodes stop after this tick                           */
    int32_t fail_ppm;   /* failure fraction in parts per million                       */
    uint64_t seed;
    int32_t max_ticks;  /* bound for digest storage; hb must stay <= 2047 (h0+ticks)   */
    int32_t tfail;      /* TFAIL suspicion (MP1Node.h:22, unused by the reference): 0 off;
                           1..tremove-1: a member whose heartbeat is tfail or more ticks
                           old is suspected -- listed until TREMOVE but not gossiped, not
                           chosen as a peer and not counted (DESIGN.md "Scale mode")   */
    int32_t swim;       /* SWIM ping/ack probing (spec p.3, not in the reference): 0 off;
                           s = 1..8: each node probes one member per tick over 1 direct +
                           s - 1 indirect paths; answered -> ts refreshed, unanswered ->
                           removed at the next tick (DESIGN.md "Scale mode"); every
                           layout                                                      */
    gsp_policy policy;  /* join schedule + bounded introducer list, drop window, crash
                           events (all zero: off)                                      */
    int32_t events;     /* event stream (Log.cpp:116-130's lines at scale), drained with
                           gsp_scale_drain_events: 0 off, GSP_EVENTS_ALL, or an OR of
                           GSP_EVENTS_JOIN / GSP_EVENTS_REMOVE                          */
    int64_t event_cap;  /* ring capacity in events (0: 2^24; rounded up to a multiple of
                           256, split evenly over 256 stripes)                          */
} gsp_scale_params;

/* params.events: which records the tick kernels keep (bit k = record kind k) */
#define GSP_EVENTS_ALL 1      /* every kind the engine has                              */
#define GSP_EVENTS_JOIN 2     /* kind 1: r added x (MP1Node.cpp:276, 297)               */
#define GSP_EVENTS_REMOVE 4   /* kind 2: r removed x after TREMOVE (MP1Node.cpp:343)    */
#define GSP_EVENTS_EVICT 8    /* kind 3: r's bounded view evicted x (partial view only) */

typedef struct {
    int64_t tick, node_rounds, merges, sent, dropped, delivered, joins, removes;
    uint64_t event_hash;   /* sum over events of mix64(kind, t, r, x), order independent */
} gsp_scale_digest;

typedef struct {
    int64_t ticks;            /* ticks stepped                                        */
    int64_t merge_launches;   /* fused tick-kernel launches timed                     */
    double merge_ms;          /* sum of fused tick-kernel durations (HIP events)      */
    double csr_ms;            /* sum of CSR build kernel durations                    */
    double bytes_per_tick;    /* algorithmic HBM bytes of the fused kernel, last tick  */
    double xgmi_bytes;        /* bytes this engine's shards sent to other shards, summed
                                 over ticks (0 on one GPU)                              */
} gsp_scale_perf;

/* Scale parameters from a .conf: the reference's four keys exactly as Params::setparams reads
 * them (Params.cpp:22-25; every reference testcase parses unchanged) mapped as its driver uses
 * them -- n = MAX_NNB, SINGLE_FAILURE 1: one Philox-chosen node crashes at t = 100, 0: n/2
 * contiguous nodes (Application.cpp:180-196), DROP_MSG: drop_pct = (int)(MSG_DROP_PROB * 100)
 * for the sends of ticks [51, 301) (EmulNet.cpp:91; Application.cpp:177/198 set and clear
 * dropmsg at the end of t = 50 / 300), STEP_RATE 0.25, 700 ticks -- then
 * optional "KEY: value" lines: SCALE_N FANOUT TREMOVE TFAIL SWIM H0 SEED TICKS STEP_RATE
 * INTRO_LIST DROP_PCT DROP_WINDOW(from until) FAIL(tick mode ppm, repeatable) EVENTS EVENT_CAP,
 * and for the partial view VIEW INBOX.  Unknown keys fail with GSP_ERR_INVALID. */
int gsp_scale_params_from_conf(const char *path, gsp_scale_params *out);
/* sizeof of a public struct by name ("gsp_scale_params", ...; 0 if unknown): lets a binding
 * check its layout */
int64_t gsp_struct_size(const char *name);

/* Single-GPU engine on `device` (rows [0, n), full rows, fused tick kernel). */
int gsp_scale_create(const gsp_scale_params *p, int device, gsp_scale **out);

/* Column-sharded job (DESIGN.md "Multi-GPU").  Shard g of G owns columns
 * [g * W, (g + 1) * W) of every row (W = n rounded up to 2048 * G, divided by G); per tick
 * the shards exchange only per-row member counts (all-gather) and the resolved peer
 * choices (all-reduce MAX).
 *   gsp_scale_nccl_id      rank 0 makes the RCCL unique id (NCCL_UNIQUE_ID_BYTES = 128);
 *                          the caller broadcasts it (e.g. torch.distributed) to every rank
 *   gsp_scale_create_rank  one process per GPU: this process holds shard `rank` of `world`
 *   gsp_scale_create_group every shard inside this process on one device, exchanged by
 *                          device copies (the same kernels and protocol, for testing the
 *                          sharded path on a single GPU)
 * Results are identical to gsp_scale_create for any number of shards. */
int gsp_scale_nccl_id(void *out, size_t cap);
int gsp_scale_create_rank(const gsp_scale_params *p, int device, int32_t rank, int32_t world,
                          const void *nccl_id, gsp_scale **out);
int gsp_scale_create_group(const gsp_scale_params *p, int device, int32_t shards,
                           gsp_scale **out);
/* One process per GPU with `tiles` column tiles per rank: the job has world * tiles column
 * shards, rank r holds shards [r * tiles, (r + 1) * tiles) and runs them as one GPU's tiles
 * (shared CSR / counts / picks, DESIGN.md "Column tiles"); the ranks exchange the counts of
 * their tiles (all-gather) and the picks (all-reduce MAX) over RCCL.  Results are identical to
 * gsp_scale_create. */
int gsp_scale_create_rank_tiled(const gsp_scale_params *p, int device, int32_t rank, int32_t world,
                                int32_t tiles, const void *nccl_id, gsp_scale **out);
/* Sharding layout of a multi-shard job.
 *   GSP_SHARD_COLUMNS  shard g owns a column slice of every row (above; O(n) exchange)
 *   GSP_SHARD_ROWS     shard g owns rows [floor(g n / G), floor((g + 1) n / G)); each tick the
 *                      sender rows that messages carry to another shard move there once per
 *                      (sender, shard) by RCCL send/recv, with the message records, and the
 *                      member counts of every row are broadcast (DESIGN.md "Multi-GPU").
 * Results are identical to gsp_scale_create in both layouts.  In the row layout
 * gsp_scale_row / gsp_scale_own_hb fail with GSP_ERR_INVALID for a row another rank holds and
 * gsp_scale_messages returns the slots of the rows held here, in row order. */
typedef enum { GSP_SHARD_COLUMNS = 0, GSP_SHARD_ROWS = 1 } gsp_shard_layout;
int gsp_scale_create_rank_layout(const gsp_scale_params *p, int device, int32_t rank,
                                 int32_t world, const void *nccl_id, int32_t layout, gsp_scale **out);
int gsp_scale_create_group_layout(const gsp_scale_params *p, int device, int32_t shards,
                                  int32_t layout, gsp_scale **out);
/* shards of the job, first shard index held by this engine, columns per shard (row layout:
 * the full row stride) */
int gsp_scale_layout(gsp_scale *s, int32_t *shards, int32_t *rank, int64_t *stride);
/* the tick form fixed at create: *width = columns per sub-slab of the tile sweep (0: one
 * workgroup per row), *seg = messages a row may have before the sweep defers it */
int gsp_scale_sweep(gsp_scale *s, int32_t *width, int32_t *seg);
int gsp_scale_destroy(gsp_scale *s);
/* Advance `ticks` ticks on the device (no host synchronisation inside). */
int gsp_scale_step(gsp_scale *s, int32_t ticks);
/* Wait for all submitted work. */
int gsp_scale_sync(gsp_scale *s);
/* Current tick (last completed). */
int gsp_scale_tick(gsp_scale *s, int32_t *tick);
/* Digest of tick t (1 <= t <= current tick). */
int gsp_scale_digest_get(gsp_scale *s, int32_t t, gsp_scale_digest *out);
/* Row r of the current table, packed entries (hb << 5 | ts mod 32; 0 = absent). */
int gsp_scale_row(gsp_scale *s, int32_t r, uint16_t *buf, int32_t cap);
int gsp_scale_own_hb(gsp_scale *s, int32_t r, int32_t *hb);
/* Surviving messages sent at the current tick: dst per (src, k) slot, -1 = none/dropped. */
int gsp_scale_messages(gsp_scale *s, int32_t *dst, int64_t cap, int64_t *n);
int gsp_scale_perf_get(gsp_scale *s, gsp_scale_perf *out);
/* Enable/disable per-launch HIP event timing (default on). */
int gsp_scale_set_timing(gsp_scale *s, int32_t on);
/* Cache policy of the row streams of the fused tick kernel: bit 0 = non-temporal loads
 * and stores of the receiver's own row, bit 1 = non-temporal loads of sender rows, bit 2 =
 * software-pipelined chunk loads (with bit 0 and the packed merge; default 5).
 * Results are identical for every policy; only speed differs. */
int gsp_scale_set_cache_policy(gsp_scale *s, int32_t policy);
/* Merge arithmetic: 1 = packed 16-bit (two entries per v_pk_* instruction, default),
 * 0 = one entry at a time.  Identical results. */
int gsp_scale_set_merge(gsp_scale *s, int32_t packed);
/* The hipStream_t (as void*) every launch of this engine is ordered on, so a caller can
 * bracket a timed region with its own HIP events on the same stream. */
int gsp_scale_hip_stream(gsp_scale *s, void **stream);

/* ------------------------------------------------------------------------------------
 * Membership census: the Grader's questions (did everyone join, was every crashed node removed
 * by everyone, was no live node removed) asked of the tables in HBM at the engine's current tick
 * T -- every tick submitted so far; valid at T = 0.  One streaming pass per call, no events
 * needed, nothing added to create or step.  A row r is alive at T iff start[r] <= T <= crash[r];
 * rows that are not alive are skipped (a crashed row's buffer is stale).  For every member x,
 * buffers of n elements each, any of them NULL:
 *   listed[x]   alive rows whose list holds x (entries as stored: no row lists itself)
 *   fresh[x]    the same, counting only entries with (T - ts) mod 32 < age_limit (1..32; 32:
 *               fresh == listed)
 *   max_hb[x]   the largest heartbeat those rows store for x (0 when listed[x] is 0)
 *   state[x]    0 not started yet, 1 alive at T, 2 crashed: the engine's own schedule
 * The arrays are the same for every layout and number of shards.  With a communicator
 * (gsp_*_create_rank*) the call is COLLECTIVE: each rank counts the rows and columns it holds
 * and the arrays are all-reduced on the engine's stream, so every rank must make the call at
 * the same tick, and every rank gets the whole result.  A pending capacity error returns
 * GSP_ERR_CAPACITY as the other reads do.  The accumulators (12 B per node) are allocated by
 * the first call and freed at destroy.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t tick, n, age_limit;
    int32_t alive;        /* nodes with state 1                                   */
    int64_t entries;      /* sum of listed[]                                      */
    double kernel_ms;     /* HIP events around the census kernels (0: timing off) */
} gsp_census_info;

int gsp_scale_census(gsp_scale *s, int32_t age_limit, uint32_t *listed, uint32_t *fresh,
                     uint32_t *max_hb, uint8_t *state, gsp_census_info *info);

/* ------------------------------------------------------------------------------------
 * View audit: the row-wise twin of the census -- what is wrong with each observer's view, and
 * do the live nodes agree -- asked of the tables in HBM at the engine's current tick T (every
 * tick submitted so far; valid at T = 0).  One streaming pass per call, nothing added to create
 * or step.  A row r is alive at T iff start[r] <= T <= crash[r]; only alive rows are read (a
 * crashed row's buffer is stale) and a row that is not alive gets 0 in every array.  For an
 * entry a view stores, age = (T - ts) mod 32.  For every alive observer r, over the entries its
 * view stores, buffers of n elements each, any of them NULL:
 *   size[r]     entries stored
 *   dead[r]     entries whose member is not alive at T (r's completeness debt)
 *   suspect[r]  entries of alive members with age >= age_limit (1..32; 32: always 0)
 *   age_sum[r]  sum of the age over the entries of alive members
 *   age_max[r]  the largest such age: tremove - 1 - age_max[r] is r's margin before it removes a
 *               live member
 *   print[r]    the fingerprint of view(r) + {r}: the sum mod 2^64 of fp(x) over those ids, fp
 *               the splitmix64 finaliser (z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) *
 *               0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; fp = z ^ z >> 31).
 *               No view stores its owner, so fp(r) is added: two nodes with the same knowledge
 *               have the same print.  A 64-bit sum can collide: equal prints are a fingerprint
 *               of agreement, not a proof.
 *   state[r]    0 not started yet, 1 alive at T, 2 crashed, as in the census
 * The arrays are the same for every layout and number of shards.  With a communicator
 * (gsp_*_create_rank*) the call is COLLECTIVE, like the census: each rank audits the rows and
 * columns it holds and the arrays are all-reduced on the engine's stream (SUM; MAX for age_max),
 * so every rank must make the call at the same tick, and every rank gets the whole result.  A
 * pending capacity error returns GSP_ERR_CAPACITY as the other reads do.  The accumulators (28 B
 * per node, and the call's truth: 1 bit per node, full view 8 B more) are allocated by the first
 * call and freed at destroy.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t tick, n, age_limit;
    int32_t alive;        /* nodes with state 1                                  */
    int64_t entries;      /* sum of size[]                                       */
    double kernel_ms;     /* HIP events around the audit kernels (0: timing off) */
} gsp_audit_info;

int gsp_scale_audit(gsp_scale *s, int32_t age_limit, uint32_t *size, uint32_t *dead,
                    uint32_t *suspect, uint32_t *age_sum, uint8_t *age_max, uint64_t *print,
                    uint8_t *state, gsp_audit_info *info);

/* ------------------------------------------------------------------------------------
 * Overlay reach: hop counts over the membership graph of the engine's current tick T (every
 * tick submitted so far; valid at T = 0), by a level-synchronous BFS on the tables in HBM.
 * Nothing is added to create or step.  Vertices are the nodes alive at T (the census's rule:
 * start[r] <= T <= crash[r]).  r -> x is an edge iff r and x are both alive, r's list holds x
 * and (T - ts) mod 32 < age_limit (1..32; 32: every stored entry).  Rows that are not alive
 * are never read, and entries for crashed members are not edges.
 *   direction   GSP_REACH_FROM: hops[x] = fewest edges from any source to x (how soon what the
 *               sources know can reach x); GSP_REACH_TO: hops[r] = fewest edges from r to any
 *               source (whose gossip can reach the sources)
 *   sources     n_sources ids in [0, n), the level-0 set; duplicates allowed, a source that is
 *               not alive at T is ignored.  With no alive source the call succeeds: every hop
 *               is -1, reached = 0, depth = -1.
 *   hops[x]     n elements: -1 for every node that is not alive or not reached
 *   state[x]    n elements, as in the census: 0 not started yet, 1 alive at T, 2 crashed
 * hops, state and info may each be NULL.  The result is the same for every layout and number
 * of shards.  One launch per local shard and level plus one host wait per level; a level costs
 * about its frontier, not the table.  With a communicator the call is COLLECTIVE: hops is
 * all-reduced (MIN) after every level, so every rank must make the call at the same tick with
 * the same arguments, and every rank gets the whole result.  A pending capacity error returns
 * GSP_ERR_CAPACITY as the other reads do.  The state (4 B + 2 bits per node) is allocated by
 * the first call and freed at destroy.
 * ---------------------------------------------------------------------------------- */
#define GSP_REACH_FROM 0
#define GSP_REACH_TO   1
typedef struct {
    int32_t tick, n, age_limit, direction;
    int32_t alive;      /* nodes alive at T                                       */
    int32_t sources;    /* distinct alive sources (level 0)                       */
    int32_t reached;    /* nodes with hops >= 0, sources included                 */
    int32_t depth;      /* largest hops value; -1 with no alive source            */
    int32_t levels;     /* level launches made (depth + 1: the last reaches none) */
    int64_t sum_hops;   /* sum of hops over reached nodes                         */
    double kernel_ms;   /* HIP events around the seeding and the whole level loop,
                           host waits between levels included (0: timing off)     */
} gsp_reach_info;

int gsp_scale_reach(gsp_scale *s, int32_t direction, int32_t age_limit, const int32_t *sources,
                    int32_t n_sources, int32_t *hops, uint8_t *state, gsp_reach_info *info);

/* ------------------------------------------------------------------------------------
 * Multi-source reach: up to 64 exact single-source BFS trees in one sweep of the tables per
 * level.  Graph, vertices, edge rule, direction, the age_limit range, aliveness and collectivity
 * are those of "Overlay reach" above.  A node's state is one 64-bit word and bit b belongs to
 * sources[b] alone: row b of every output equals what gsp_*_reach returns for the one-element
 * source set {sources[b]}, at the cost of about one streaming pass per level for all trees.
 *   sources     n_sources (1..GSP_REACH_MAX_SOURCES) ids in [0, n).  The same id may stand under
 *               several bits; those bits get equal rows.  A source that is not alive at T leaves
 *               its row empty: hops -1, reached 0, ecc -1, sum_hops 0.
 *   seen[x]     n elements: bit b set iff x is reached from (FROM) / reaches (TO) sources[b]; the
 *               source itself counts, at hop 0
 *   hops[b * n + x]   int32, -1 where x is not alive or not reached by tree b
 *   reached[b], ecc[b], sum_hops[b]   n_sources elements each: the nodes tree b reached, its
 *               largest hop count, and the sum of its hops
 *   level_sizes[b * level_cap + l]   for l < level_cap: the nodes at hop l of tree b (0 past its
 *               ecc).  Levels >= level_cap are dropped from this array only.
 *   state[x]    n elements, as in the census
 * Any output may be NULL.  The result is the same, bit for bit, for every layout and number of
 * shards: a level's launches only read what the previous level left and only OR into the next
 * frontier.  One launch per local shard and level plus one host wait per level, for all trees
 * together.  With a communicator the call is COLLECTIVE like gsp_*_reach: the next frontier of
 * every rank is all-gathered and ORed after every level, and every rank gets the whole result.
 * A bad argument returns GSP_ERR_INVALID before any launch; a pending capacity error returns
 * GSP_ERR_CAPACITY as the other reads do.  The state (24 B + 2 bits per node; 4 B per node and
 * source more once a call asks for hops) is allocated by the first call and freed at destroy.
 * ---------------------------------------------------------------------------------- */
#define GSP_REACH_MAX_SOURCES 64
typedef struct {
    int32_t tick, n, age_limit, direction;
    int32_t alive;          /* nodes alive at T                                        */
    int32_t n_sources;      /* as passed                                               */
    int32_t alive_sources;  /* bits whose source is alive at T                         */
    int32_t depth;          /* largest hop count over all sources; -1: no alive source */
    int32_t levels;         /* level launches made                                     */
    int32_t reserved;
    int64_t pairs;          /* sum over sources of the nodes reached, source included  */
    int64_t sum_hops;       /* sum of hops over those pairs                            */
    double kernel_ms;       /* as gsp_reach_info                                       */
} gsp_reach_multi_info;

int gsp_scale_reach_multi(gsp_scale *s, int32_t direction, int32_t age_limit,
                          const int32_t *sources, int32_t n_sources,
                          uint64_t *seen, int32_t *hops, int32_t *reached, int32_t *ecc,
                          int64_t *sum_hops, uint32_t *level_sizes, int32_t level_cap,
                          uint8_t *state, gsp_reach_multi_info *info);

/* ------------------------------------------------------------------------------------
 * Overlay clustering: for up to 64 observers at once, how many of an observer's neighbours list
 * each other and how many list the observer back.  Graph, vertices, edge rule, the age_limit
 * range, aliveness and collectivity are those of "Overlay reach" above; bit b belongs to
 * observers[b] alone, as in "Multi-source reach".  For an alive observer o = observers[b] with
 * out-neighbour set N = {x : o -> x}:
 *   observers   n_observers (1..GSP_CLUSTER_MAX_OBSERVERS) ids in [0, n).  The same id may stand
 *               under several bits; those bits get equal results.  An observer that is not alive
 *               at T gets zeros, and its bit is set nowhere.
 *   member[x]   n elements: bit b set iff x is in N
 *   degree[b]   |N|
 *   links[b]    the ordered pairs (u, v) with u in N, v in N and u -> v, i.e. the sum over u in N
 *               of |N(u) & N|: k (k - 1) where N is a clique, 0 where no two neighbours list each
 *               other.  64-bit: it passes 2^32 at 65,536 nodes.
 *   mutual[b]   the u in N with u -> o
 *   state[x]    n elements, as in the census
 * The local clustering coefficient of observers[b] is links[b] / (degree[b] (degree[b] - 1)).
 * Any output may be NULL.  Every output is an integer built by OR and ADD alone, the same bit for
 * bit for every layout and number of shards.  Two phases with the kernel boundary between them:
 * the observers' rows are walked into member, then the rows with a non-zero member word are
 * walked once (the full view: one streaming pass over those rows of the table).  With a
 * communicator the call is COLLECTIVE: member is all-reduced between the phases and the counters
 * after them, and every rank gets the whole result.  A bad argument returns GSP_ERR_INVALID
 * before any launch; a pending capacity error returns GSP_ERR_CAPACITY as the other reads do.
 * The state (8 B + 1 bit per node, and 96 KiB of counters) is allocated by the first call and
 * freed at destroy.
 * ---------------------------------------------------------------------------------- */
#define GSP_CLUSTER_MAX_OBSERVERS 64
typedef struct {
    int32_t tick, n, age_limit;
    int32_t alive;            /* nodes alive at T                                          */
    int32_t n_observers;      /* as passed                                                 */
    int32_t alive_observers;  /* bits whose observer is alive at T                         */
    int32_t rows;             /* nodes whose member word is non-zero: the rows phase 2 walks */
    int32_t reserved;
    int64_t sum_degree;       /* sums over the bits                                        */
    int64_t sum_links;
    int64_t sum_mutual;
    double kernel_ms;         /* HIP events around both phases (0: timing off)             */
} gsp_cluster_info;

int gsp_scale_cluster(gsp_scale *s, int32_t age_limit, const int32_t *observers,
                      int32_t n_observers, uint64_t *member, uint32_t *degree, uint64_t *links,
                      uint32_t *mutual, uint8_t *state, gsp_cluster_info *info);

/* ------------------------------------------------------------------------------------
 * Overlay components: the exact weakly or strongly connected components of the overlay, i.e.
 * how many pieces it has fallen into, how large each is and which one a node is in.  Graph,
 * vertices, edge rule, the age_limit range (1..32), aliveness and collectivity are those of
 * "Overlay reach" above: r -> x is an edge iff r and x are both alive at T, r's list holds x and
 * (T - ts) mod 32 < age_limit.
 *   kind        GSP_COMPONENTS_WEAK: the components of the undirected graph that has an edge
 *               wherever either endpoint lists the other; GSP_COMPONENTS_STRONG: the strongly
 *               connected components of the directed graph
 *   label[x]    n elements, int32: for an alive x the smallest node id of x's component, -1 for a
 *               node that is not alive.  This form does not depend on the order atomics land in,
 *               on the layout or on the algorithm.
 *   state[x]    n elements, as in the census
 *   max_sweeps  a cap on table sweeps (one sweep: one pass of every local shard over its rows);
 *               0 selects GSP_COMPONENTS_DEFAULT_SWEEPS.  Negative values are invalid.  When the
 *               cap ends the loop early the call still returns GSP_OK, with info.converged = 0
 *               and label unspecified for alive nodes.
 * label, state and info may each be NULL.  The result is the same for every layout and number of
 * shards.  A round is one sweep per local shard, one n-length kernel and one host wait; weak
 * hooks tree roots under smaller roots and jumps pointers until a round changes nothing, strong
 * trims and colours forwards and backwards on the nodes not yet assigned (components_kernels.hpp).
 * With a communicator the call is COLLECTIVE: the label arrays are all-reduced (MIN / MAX) after
 * every sweep, and every rank gets the whole result.  A bad argument returns GSP_ERR_INVALID
 * before any launch; a pending capacity error returns GSP_ERR_CAPACITY as the other reads do.
 * The state (32 B + 1 bit per node) is allocated by the first call and freed at destroy.
 * ---------------------------------------------------------------------------------- */
#define GSP_COMPONENTS_WEAK   0
#define GSP_COMPONENTS_STRONG 1
#define GSP_COMPONENTS_DEFAULT_SWEEPS 65536
typedef struct {
    int32_t tick, n, age_limit, kind;
    int32_t alive;          /* nodes alive at T                                            */
    int32_t components;     /* distinct labels                                             */
    int32_t largest;        /* nodes of the largest component; 0 with no alive node        */
    int32_t largest_label;  /* its label (the smallest among equals); -1 with no alive node */
    int32_t singletons;     /* components of one node                                      */
    int32_t sweeps;         /* table sweeps made                                           */
    int32_t rounds;         /* host waits made                                             */
    int32_t converged;      /* 0: max_sweeps ended the loop; the four counts above are 0 / -1 */
    double kernel_ms;       /* as gsp_reach_info                                           */
} gsp_components_info;

int gsp_scale_components(gsp_scale *s, int32_t kind, int32_t age_limit, int32_t max_sweeps,
                         int32_t *label, uint8_t *state, gsp_components_info *info);

/* ------------------------------------------------------------------------------------
 * Rumor trace: dissemination times over the messages the engine really delivers.  A trace
 * carries up to 32 independent rumors, the bits of one 32-bit word per node; while one is open,
 * every tick adds one small pull kernel per local shard over the tick's receiver CSR (JOINREPs
 * included), ahead of the tick kernels.  With no trace open nothing is added to create or step.
 *   know_t[x]   the rumors node x has heard by the end of tick t
 *   heard[b][x] the tick at which bit b of know[x] was first set, -1 if never
 * Alive at t is the census's rule, start[x] <= t <= crash[x].
 *   seed    between steps, at the engine's tick T: every source alive at T gets bit `rumor`, and
 *           heard = T where it was unset.  Duplicates and sources that are not alive are ignored;
 *           a later seed of the same rumor adds sources.
 *   tick t  a receiver r alive at t hears the OR of know_{t-1}[s] over the senders s whose
 *           messages it merges at t -- every entry of its segment (full view; partial view with
 *           inbox 0), or the `inbox` smallest senders of it (bounded partial view).  A JOINREP
 *           rides like a GOSSIP from node 0, sorts first and takes an inbox slot.  know_t[r] =
 *           know_{t-1}[r] | heard, and every bit newly set gives heard[b][r] = t.  A row that is
 *           not alive at t keeps its mask.  Senders are read from know_{t-1} only: news moves one
 *           hop per tick.  SWIM probes and TFAIL carry nothing.
 * open     rumors in 1..32; an error while a trace is open.  Allocates know[2][n], heard[rumors][n]
 *          and known[rumors][max_ticks + 1] on the device.
 * get      synchronises (a pending capacity error returns GSP_ERR_CAPACITY as the other reads
 *          do).  heard: n elements; state: n elements as in the census; known[t] for t <
 *          min(known_cap, T + 1): the nodes whose heard[rumor] equals t, counted on the device.
 *          Any pointer may be NULL.
 * close    frees the trace; step is back to the launches it makes without one.
 * The result is the same for every layout and number of shards.  With a communicator open,
 * seed, get and close are COLLECTIVE (row shards all-reduce know each tick and heard / known at
 * get), so every rank makes them at the same tick with the same arguments.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t tick, n, rumor;
    int32_t seed_tick;    /* tick of the first seed with an alive source, -1: none yet     */
    int32_t sources;      /* distinct sources that were alive when they were seeded        */
    int32_t alive;        /* nodes alive at T                                              */
    int32_t known;        /* nodes with heard >= 0                                         */
    int32_t known_alive;  /* ... that are alive at T                                       */
    int32_t last_heard;   /* largest heard value, -1 if nobody heard                       */
    int32_t ticks_traced; /* ticks stepped since open                                      */
    double kernel_ms;     /* HIP events around every tick's trace launches since open,
                             collected at sync (0: timing off)                             */
} gsp_rumor_info;

int gsp_scale_rumor_open(gsp_scale *s, int32_t rumors);
int gsp_scale_rumor_seed(gsp_scale *s, int32_t rumor, const int32_t *sources, int32_t n_sources);
int gsp_scale_rumor_get(gsp_scale *s, int32_t rumor, int32_t *heard, uint8_t *state,
                        int32_t *known, int32_t known_cap, gsp_rumor_info *info);
int gsp_scale_rumor_close(gsp_scale *s);

/* ------------------------------------------------------------------------------------
 * Event stream (params.events != 0): the tick kernels append every join / remove (partial
 * view: and evict) of the selected kinds as one 64-bit record kind << 62 | t << 42 | r << 21
 * | x (kind 1 join, 2 remove, 3 evict; r = the node whose list changed, x = the member) --
 * the scale form of Log::logNodeAdd / logNodeRemove (Log.cpp:116-130).  A row's records are
 * staged in LDS and reserved in the ring at once; the ring is 256 stripes (row % 256), each
 * with its own counter, so reservations do not queue on one address.
 * drain: copies the records of every tick since the last drain (stripe by stripe, device
 * order within a stripe) into buf, at most cap of them, sets *n to the number copied and
 * *lost to the records a full stripe could not hold plus those past cap, and empties the
 * ring; buf = NULL only counts (*n = the records held; the ring is kept).
 * ---------------------------------------------------------------------------------- */
int gsp_scale_drain_events(gsp_scale *s, uint64_t *buf, int64_t cap, int64_t *n, int64_t *lost);
/* Appends event records as the reference's dbg.log lines (Log.cpp:44-130): "\n <r> [t] Node
 * <x> joined at time t" ("removed", "evicted"), addresses printed as Log.cpp:73 does (id =
 * index + 1 in signed bytes, port 0), in a canonical order -- t ascending, r descending (the
 * phase-P order of Application.cpp:138), joins then removes then evictions, x ascending.  A
 * new file starts with the "131" header (Log.cpp:79-88).  ev is sorted in place. */
int gsp_events_write_log(uint64_t *ev, int64_t n, const char *path);

/* ------------------------------------------------------------------------------------
 * Detection ledger: the event records folded per member on the device.  While a ledger is
 * open, every tick ends with one fold over each local shard's event ring: the tick's records
 * are reduced into the arrays below and the ring is emptied, so it never fills across ticks and
 * no record leaves the device before get.  With no ledger open nothing is added to step.
 * crash[x] is the engine's failure schedule (INT32_MAX: never); by the census's aliveness rule
 * x is alive at t while t <= crash[x].  Per member x, n elements each:
 *   first_remove / last_remove  smallest / largest t over remove records of x with t > crash[x],
 *                               -1: none
 *   removers                    how many such records
 *   false_removes / first_false remove records of x with t <= crash[x] (x was alive at t): how
 *                               many, and the smallest t (-1: none)
 *   revivals                    join records of x with t > crash[x]
 *   evicts                      evict records of x (all 0 in the full view)
 *   state                       as in the census, at the engine's tick T
 * by_tick[t][4] for t < min(by_tick_cap, T + 1): the true removes, false removes, revivals and
 * evictions whose record tick is t.  Any out pointer may be NULL.
 * open     GSP_ERR_INVALID when the engine does not record removes (params.events) or a ledger
 *          is open.  Folds what the ring holds at that moment -- every record since the last
 *          drain: opened at tick 0 a ledger covers the run, opened after a drain at tick T it
 *          covers the ticks > T.  Kinds the engine does not record count 0.
 * fold     each fold adds max(0, counter - stripe capacity) per stripe to `lost`, the records a
 *          full stripe refused within that tick: records + lost = the records the tick kernels
 *          made.  gsp_*_drain_events is unchanged; after a step it finds an empty ring.
 * get      synchronises (a pending capacity error returns GSP_ERR_CAPACITY as the other reads do).
 * close    frees the ledger and leaves the ring empty; it fills and drains as before from then on.
 * The result is the same for every layout and number of shards.  With a communicator open, get
 * and close are COLLECTIVE (get all-reduces MIN / MAX / SUM into a staging buffer).
 * ---------------------------------------------------------------------------------- */
typedef struct {
    int32_t tick, n;
    int32_t open_tick;     /* the engine's tick at open                                     */
    int32_t kinds;         /* the kinds the engine records: an OR of GSP_EVENTS_JOIN / REMOVE /
                              EVICT                                                         */
    int32_t ticks_folded;  /* ticks stepped since open (one fold each)                      */
    int32_t reserved;
    int64_t records;       /* records folded                                                */
    int64_t lost;          /* records a full stripe refused                                 */
    int64_t true_removes, false_removes, joins, revivals, evicts;
    double kernel_ms;      /* HIP events around every fold since open, collected at sync (0:
                              timing off)                                                   */
} gsp_detect_info;

int gsp_scale_detect_open(gsp_scale *s);
int gsp_scale_detect_get(gsp_scale *s, int32_t *first_remove, int32_t *last_remove,
                         uint32_t *removers, uint32_t *false_removes, int32_t *first_false,
                         uint32_t *revivals, uint32_t *evicts, uint8_t *state, uint64_t *by_tick,
                         int32_t by_tick_cap, gsp_detect_info *info);
int gsp_scale_detect_close(gsp_scale *s);

/* ------------------------------------------------------------------------------------
 * Traffic ledger: per-node message and payload load, counted on the device -- the scale form
 * of the reference's sent_msgs / recv_msgs (EmulNet.cpp:111, :172) and of msgcount.log.  While a
 * ledger is open every tick runs two small passes: one over the tick's receiver CSR before the
 * tick kernels, one over the tick's send slots once they are final.  With no ledger open nothing
 * is added to step.
 * A ledger opened at engine tick T0 covers the sends made and the messages taken at ticks t in
 * (T0, T], T the engine's tick at get.  x is alive at t while start[x] <= t <= crash[x] (the
 * census's rule).  Per node, n elements each:
 *   sent[x]       messages x put on the network: the sends that survived the drop test, counted
 *                 at the tick they are sent; a delivered JOINREP counts for node 0
 *   recv[r]       messages addressed to r at a tick at which r is alive, before any inbox cut (a
 *                 JOINREP is one message)
 *   merged[r]     of those, the ones r merges: all of them in the full view and with inbox = 0,
 *                 else the `inbox` smallest senders (a JOINREP first); recv - merged is the inbox
 *                 overflow at r
 *   lost[r]       messages addressed to r at a tick at which r is not alive
 *   entries_in[r] over r's merged messages, 1 + payload entries -- r's share of the digest's
 *                 merges.  A GOSSIP from s carries s's gossipable members at the send tick (TFAIL
 *                 suspects left out), a JOINREP min(intro_list, node 0's gossipable members)
 *   peak_recv[r], peak_tick[r]  the largest recv of one tick and the first tick it occurred (-1:
 *                 r received nothing)
 *   state         as in the census, at T
 * Per tick t < min(tick_cap, T + 1):
 *   by_tick[t][6] sent, recv, merged, lost, entries and the largest recv of that tick
 *   fanin[t][18]  the receivers alive at t by the messages k they were sent: bucket 0 holds k = 0,
 *                 bucket b >= 1 holds 2^(b-1) <= k < 2^b, the last bucket is open-ended
 *   watch[w][t][2]  (sent, recv) of the w-th watched node at t; the caller's array is
 *                 [n_watch][tick_cap][2]
 * Rows of ticks outside (T0, T] are 0.  Any out pointer may be NULL.
 * open     watch: up to 1,024 distinct node ids in [0, n) (NULL with n_watch = 0: none);
 *          GSP_ERR_INVALID otherwise, and while a ledger is open.
 * get      synchronises (a pending capacity error returns GSP_ERR_CAPACITY as the other reads do).
 * close    frees the ledger; step is back to the launches it makes without one.
 * The result is the same for every layout and number of shards.  With a communicator open, get
 * and close are COLLECTIVE (row shards all-reduce SUM / MAX into a staging buffer at get).
 * ---------------------------------------------------------------------------------- */
#define GSP_TRAFFIC_BUCKETS 18
#define GSP_TRAFFIC_MAX_WATCH 1024

typedef struct {
    int32_t tick, n;
    int32_t open_tick;     /* the engine's tick at open                                     */
    int32_t ticks_counted; /* ticks stepped since open                                      */
    int32_t n_watch;
    int32_t reserved;
    int64_t sent, recv, merged, lost, entries, overflow;   /* over the ticks in (T0, T]     */
    int32_t max_fanin;     /* the largest recv of one node and tick                         */
    int32_t max_fanin_node;/* the node that took it: first tick, then smallest id; -1: none */
    double kernel_ms;      /* HIP events around every tick's ledger launches since open,
                              collected at sync (0: timing off)                             */
} gsp_traffic_info;

int gsp_scale_traffic_open(gsp_scale *s, const int32_t *watch, int32_t n_watch);
int gsp_scale_traffic_get(gsp_scale *s, uint32_t *sent, uint32_t *recv, uint32_t *merged,
                          uint32_t *lost, uint64_t *entries_in, uint32_t *peak_recv,
                          int32_t *peak_tick, uint8_t *state, uint64_t *by_tick, uint64_t *fanin,
                          uint32_t *watch, int32_t tick_cap, gsp_traffic_info *info);
int gsp_scale_traffic_close(gsp_scale *s);
/* Writes `nodes` rows of `ticks` columns (sent[i * ticks + j], recv[i * ticks + j]) as the
 * reference's msgcount.log (EmulNet.cpp:195-216): the rows are numbered node 1..nodes, ten pairs
 * per line, node 67 in the reference's "special" layout.  gsp_write_msgcount prints the exact
 * engine's counters through the same formatter. */
int gsp_traffic_write_msgcount(const char *path, const int32_t *sent, const int32_t *recv,
                               int32_t nodes, int32_t ticks);

/* ------------------------------------------------------------------------------------
 * PARTIAL-VIEW engine (BASELINE config 5): every node keeps at most `view` member entries
 * (id, hb, ts) sorted by id; a receiver merges at most `inbox` messages per tick (1..7,
 * ascending sender; the rest are counted as overflow) -- or, with inbox = 0, every message it
 * was sent, as the reference's checkMessages drains its queue (MP1Node.cpp:200-212; every
 * protocol option, for n <= 2^21 - 768: the hub kernel's buffers hold any receiver's list);
 * after the TREMOVE scan a view larger than `view` keeps the entries with the smallest
 * (age, -hb, id).  DESIGN.md "Partial view".
 * ---------------------------------------------------------------------------------- */
typedef struct gsp_pview gsp_pview;

typedef struct {
    int32_t n, view, fanout, inbox, drop_pct, tremove, h0, fail_mode, fail_tick, fail_ppm;
    uint64_t seed;
    int32_t max_ticks;
    int32_t tfail, swim;  /* as gsp_scale_params: TFAIL suspicion, SWIM probing (0: off)   */
    gsp_policy policy;    /* as gsp_scale_params                                         */
    int32_t events;       /* as gsp_scale_params, with GSP_EVENTS_EVICT (gsp_pview_drain_events) */
    int64_t event_cap;    /* as gsp_scale_params                                          */
    int32_t evict_order;  /* 0: a view past `view` keeps the smallest (age, -hb, id) -- the
                             default, and the order every headline number is quoted on; 1:
                             ties of (age, hb) broken by the rotated id (id - m) mod n, m =
                             Philox(EVICT; t, r) mod n, so no id is favoured (the id order makes
                             low ids hubs) */
} gsp_pview_params;

typedef struct {
    int64_t tick, node_rounds, merges, sent, dropped, delivered, overflow, joins, removes, evicts;
    uint64_t event_hash;   /* sum of h(kind, t, r, x) = mix64(kind, t, r, 0) + a 3-multiply
                              finaliser of x (oracle: gsp_pv_event_mix); kinds 1 join,
                              2 remove, 3 evict */
} gsp_pview_digest;

/* As gsp_scale_params_from_conf, plus the VIEW / INBOX keys (defaults 256 / 7). */
int gsp_pview_params_from_conf(const char *path, gsp_pview_params *out);
int gsp_pview_create(const gsp_pview_params *p, int device, gsp_pview **out);
/* Row-sharded job (DESIGN.md "Partial view, row shards").  Shard g of G owns the views of
 * nodes [floor(g n / G), floor((g + 1) n / G)); per tick every sender view that a message
 * carries to another shard moves there once per (sender, shard), with the message records,
 * by RCCL send/recv (one process per GPU: gsp_pview_create_rank, RCCL id from
 * gsp_scale_nccl_id) or by device copies (gsp_pview_create_group: every shard inside this
 * process on one device, for testing the sharded path on one GPU).  Results are identical
 * to gsp_pview_create for any number of shards. */
int gsp_pview_create_rank(const gsp_pview_params *p, int device, int32_t rank, int32_t world,
                          const void *nccl_id, gsp_pview **out);
int gsp_pview_create_group(const gsp_pview_params *p, int device, int32_t shards, gsp_pview **out);
/* shards of the job, first shard held here, its first row, rows held by this engine */
int gsp_pview_layout(gsp_pview *s, int32_t *shards, int32_t *rank, int32_t *row0, int32_t *rows);
int gsp_pview_destroy(gsp_pview *s);
int gsp_pview_step(gsp_pview *s, int32_t ticks);
int gsp_pview_sync(gsp_pview *s);
int gsp_pview_digest_get(gsp_pview *s, int32_t t, gsp_pview_digest *out);
/* Row r: `view` packed entries (id << 32 | hb << 5 | ts mod 32, ~0 = empty) and its length. */
int gsp_pview_row(gsp_pview *s, int32_t r, uint64_t *buf, int32_t cap, int32_t *len);
/* gsp_pview_row / gsp_pview_own_hb fail with GSP_ERR_INVALID for a row another rank holds;
 * gsp_pview_messages returns the slots of the rows held here, in row order. */
int gsp_pview_own_hb(gsp_pview *s, int32_t r, int32_t *hb);
int gsp_pview_messages(gsp_pview *s, int32_t *dst, int64_t cap, int64_t *n);
int gsp_pview_perf_get(gsp_pview *s, gsp_scale_perf *out);
/* Drain all (inbox 0): per drain row class since create -- rows run, messages they merged and
 * kernel ms (HIP events around each class's launch; 0 with timing off) -- for `classes`
 * entries (class c < 4: the LDS classes, 4: the hub kernel; entries past them 0).  The
 * counts are read back with the split kernels' bucket sizes (the default launch form). */
int gsp_pview_drain_stats(gsp_pview *s, int32_t classes, int64_t *rows, int64_t *messages, double *ms);
/* As gsp_scale_census ("Membership census" above), over the views. */
int gsp_pview_census(gsp_pview *s, int32_t age_limit, uint32_t *listed, uint32_t *fresh,
                     uint32_t *max_hb, uint8_t *state, gsp_census_info *info);
/* As gsp_scale_audit ("View audit" above), over the views. */
int gsp_pview_audit(gsp_pview *s, int32_t age_limit, uint32_t *size, uint32_t *dead,
                    uint32_t *suspect, uint32_t *age_sum, uint8_t *age_max, uint64_t *print,
                    uint8_t *state, gsp_audit_info *info);
/* As gsp_scale_reach ("Overlay reach" above): a view is its row's out-edge list. */
int gsp_pview_reach(gsp_pview *s, int32_t direction, int32_t age_limit, const int32_t *sources,
                    int32_t n_sources, int32_t *hops, uint8_t *state, gsp_reach_info *info);
/* As gsp_scale_reach_multi ("Multi-source reach" above). */
int gsp_pview_reach_multi(gsp_pview *s, int32_t direction, int32_t age_limit,
                          const int32_t *sources, int32_t n_sources,
                          uint64_t *seen, int32_t *hops, int32_t *reached, int32_t *ecc,
                          int64_t *sum_hops, uint32_t *level_sizes, int32_t level_cap,
                          uint8_t *state, gsp_reach_multi_info *info);
/* As gsp_scale_cluster ("Overlay clustering" above); the rows walked are at most 64 x view. */
int gsp_pview_cluster(gsp_pview *s, int32_t age_limit, const int32_t *observers,
                      int32_t n_observers, uint64_t *member, uint32_t *degree, uint64_t *links,
                      uint32_t *mutual, uint8_t *state, gsp_cluster_info *info);
/* As gsp_scale_components ("Overlay components" above). */
int gsp_pview_components(gsp_pview *s, int32_t kind, int32_t age_limit, int32_t max_sweeps,
                         int32_t *label, uint8_t *state, gsp_components_info *info);
/* As gsp_scale_rumor_*("Rumor trace" above); a bounded inbox hears its `inbox` smallest senders. */
int gsp_pview_rumor_open(gsp_pview *s, int32_t rumors);
int gsp_pview_rumor_seed(gsp_pview *s, int32_t rumor, const int32_t *sources, int32_t n_sources);
int gsp_pview_rumor_get(gsp_pview *s, int32_t rumor, int32_t *heard, uint8_t *state,
                        int32_t *known, int32_t known_cap, gsp_rumor_info *info);
int gsp_pview_rumor_close(gsp_pview *s);
/* As gsp_scale_drain_events (join / remove / evict records). */
int gsp_pview_drain_events(gsp_pview *s, uint64_t *buf, int64_t cap, int64_t *n, int64_t *lost);
/* As gsp_scale_detect_* ("Detection ledger" above), with evict records. */
int gsp_pview_detect_open(gsp_pview *s);
int gsp_pview_detect_get(gsp_pview *s, int32_t *first_remove, int32_t *last_remove,
                         uint32_t *removers, uint32_t *false_removes, int32_t *first_false,
                         uint32_t *revivals, uint32_t *evicts, uint8_t *state, uint64_t *by_tick,
                         int32_t by_tick_cap, gsp_detect_info *info);
int gsp_pview_detect_close(gsp_pview *s);
/* As gsp_scale_traffic_* ("Traffic ledger" above); a bounded inbox merges its `inbox` smallest
 * senders, and with TFAIL one count pass per tick sizes the payloads while a ledger is open. */
int gsp_pview_traffic_open(gsp_pview *s, const int32_t *watch, int32_t n_watch);
int gsp_pview_traffic_get(gsp_pview *s, uint32_t *sent, uint32_t *recv, uint32_t *merged,
                          uint32_t *lost, uint64_t *entries_in, uint32_t *peak_recv,
                          int32_t *peak_tick, uint8_t *state, uint64_t *by_tick, uint64_t *fanin,
                          uint32_t *watch, int32_t tick_cap, gsp_traffic_info *info);
int gsp_pview_traffic_close(gsp_pview *s);
/* Test diagnostics: the rows the tick kernels of tick t ran, summed over the shards held here
 * -- every row exactly once in every launch form, so it equals the rows held.  Needs the
 * environment variable GSP_TEST_PV_COUNT_ROWS=1 at create (else GSP_ERR_INVALID). */
int gsp_pview_rows_run(gsp_pview *s, int32_t t, int64_t *rows);

#ifdef __cplusplus
}
#endif
#endif /* GOSSIP_GOSSIP_H */
