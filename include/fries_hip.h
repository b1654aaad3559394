/* C ABI of the MI355X-native FRI engine (libfries_hip.so).
 *
 * The reference (sgreene8/FRIES) has no FFI: its hot path is C++ called in-process through the
 * headers it installs under include/FRIES/.  Each entry point below names the reference
 * interface it stands in for; the binding a FRIES maintainer would add is shown in
 * INTEGRATION.md.  Conventions: plain pointers and sizes only, host buffers unless a name says
 * "device"; every function returns 0 on success or a negative code, and fries_last_error()
 * then holds the message (the reference throws std::runtime_error and prints it,
 * FRIES_bin/frisys_mol.cpp:562-565).  A determinant is a uint64_t whose bit i is spin orbital i
 * (alpha 0..n_orb-1, beta n_orb..2n_orb-1) -- the reference's little-endian byte string
 * (FRIES/det_store.h:23-26) for 2*n_orb <= 64.
 */
#ifndef FRIES_HIP_H
#define FRIES_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct fries_ctx fries_ctx;

const char *fries_last_error(void);
/* number of HIP devices visible; 0 means the engine cannot run (there is no CPU fallback) */
int fries_device_count(void);

int fries_ctx_create(fries_ctx **out, int device);
void fries_ctx_destroy(fries_ctx *ctx);

/* parse_fcidump's result handed to the device: FRIES/io_utils.cpp:241-318 (fcidump_input),
 * SymmERIs packing FRIES/ndarr.hpp:206-244, SymmInfo FRIES/Hamiltonians/molecule.hpp:265-280,
 * plus set_up(tot_orb, n_orb, eris) FRIES/Hamiltonians/heat_bathPP.cpp:99-179. */
int fries_set_molecule(fries_ctx *ctx, uint32_t n_orb, uint32_t n_elec, const uint8_t *irreps,
                       const double *h_core, const double *eris_packed);

/* hb_info accessors (FRIES/Hamiltonians/heat_bathPP.hpp:25-34).  which: 0 s_tens[n], 1 d_same[n(n-1)/2],
 * 2 d_diff[n*n], 3 exch_sqrt[n(n-1)/2], 4 diag_sqrt[n], 5 exch_norms[n], 6 s_norm[1]. */
int fries_get_hb_tensor(fries_ctx *ctx, int which, double *out, size_t cap, size_t *len);
int fries_set_hb_tensor(fries_ctx *ctx, int which, const double *in, size_t len);
double fries_hf_energy(fries_ctx *ctx);     /* diag_matrel of the HF determinant, frisys_mol.cpp:100 */

/* Batched Slater-Condon elements (FRIES/Hamiltonians/molecule.cpp:983-1029, 76-105, 26-42) and
 * fermionic signs (FRIES/fci_utils.c:46-96).  orbs: n x 4 bytes, (o1,o2,u1,u2) or (o,u,0,0).
 * kind: 0 diag_matrel(det), 1 sing_matr_el_nosgn, 2 doub_matr_el_nosgn; sign receives
 * sing_parity / doub_parity for kinds 1, 2. */
int fries_matrel_batch(fries_ctx *ctx, int kind, const uint64_t *dets, const uint8_t *orbs, size_t n,
                       double *out, int32_t *sign);

/* ---- ranks ------------------------------------------------------------------------------------
 * The reference shards the solution vector over MPI ranks by determinant hash (DistVec::idx_to_proc,
 * FRIES/vec_utils.hpp:360-379) and synchronises with blocking collectives on MPI_COMM_WORLD:
 * sum_mpi = MPI_Allgather + a sum in rank order (compress_utils.hpp:170-231), MPI_Alltoallv of the
 * pending adds (Adder::perform_add, vec_utils.hpp:991-1019), MPI_Allgather of the local norms
 * (compress_utils.cpp:326, :818), MPI_Bcast of rank 0's uniform (:291, :806).
 * The engine does the same with ONE process per GPU and two caller-supplied collectives that run
 * on caller-owned DEVICE staging buffers, stream-ordered like an RCCL call: when the callback
 * returns, the collective must be ordered after everything already enqueued on `stream`, and work
 * enqueued on `stream` afterwards must see its result.  fries_amd/comm.py implements them with
 * torch.distributed (backend "nccl" = RCCL over xGMI; "gloo" for tests); INTEGRATION.md shows the
 * GPU-aware-MPI version a FRIES maintainer would write. */
#define FRIES_COMM_SMALL_BYTES 2048
#define FRIES_COMM_MAX_RANKS 64
typedef struct {
    void *user;
    int32_t rank, size;
    void *small_send;       /* device, FRIES_COMM_SMALL_BYTES */
    void *small_recv;       /* device, size * FRIES_COMM_SMALL_BYTES */
    void *big_send;         /* device, big_bytes: all-to-all segments, contiguous in destination order */
    void *big_recv;         /* device, big_bytes: received segments, contiguous in source order */
    uint64_t big_bytes;
    /* every rank contributes small_send[0, bytes); rank p's block lands at small_recv + p * bytes */
    int (*allgather)(void *user, uint64_t bytes, void *stream);
    /* send_bytes[d] bytes of big_send go to rank d, recv_bytes[s] bytes arrive from rank s (host arrays of `size`) */
    int (*alltoallv)(void *user, const uint64_t *send_bytes, const uint64_t *recv_bytes, void *stream);
} fries_comm;
/* Native transports (csrc/comm_native.hip) that fill a fries_comm -- the C++ counterpart of MPI_COMM_WORLD in the reference:
 *   RCCL: one process per MI355X.  Rank 0 makes the 128-byte id (fries_rccl_unique_id) and the launcher hands it to every rank
 *   (a file, MPI_Bcast, a TCP store: the drivers use a rendezvous file); fries_rccl_create joins the communicator on `device`.
 *   The all-gather is ncclAllGather and the all-to-all ncclAllToAllv, both on the engine's stream.
 *   local: `size` ranks = `size` host threads of one process, each driving its own context, on any devices; several ranks
 *   may share one GPU (RCCL refuses that), so multi-rank runs can be checked on a one-GPU machine.  Every rank's thread must
 *   enter each collective (the engine does); create the group once, then one transport per rank.
 * big_bytes >= 16 x (mat_nonz + 4096), the same on every rank. */
typedef struct fries_transport fries_transport;
typedef struct fries_local_group fries_local_group;
int fries_rccl_unique_id(uint8_t id[128]);
int fries_rccl_create(fries_transport **out, const uint8_t id[128], int rank, int size, int device, uint64_t big_bytes);
int fries_local_group_create(fries_local_group **out, int size, uint64_t big_bytes);
void fries_local_group_destroy(fries_local_group *g);
int fries_local_create(fries_transport **out, fries_local_group *g, int rank, int device);
/*   host: the caller's own collectives on HOST buffers -- for a program that already lives in an MPI communicator (the reference's
 *   drivers call MPI directly: MPI_Allgather inside sum_mpi, MPI_Alltoallv inside Adder::perform_add).  The transport moves the staging
 *   blocks to pinned host memory, calls back, and moves the result to the device; no GPU-aware MPI is needed.  allgather: every rank
 *   contributes `bytes` bytes, rank p's block lands at recv + p * bytes.  alltoallv: send holds the segments for ranks 0 .. size-1 back to
 *   back (send_bytes[d] each), recv receives the segments from ranks 0 .. size-1 back to back (recv_bytes[s] each).  Return 0 on success.
 *   include/FRIES/backend.hpp builds these two from MPI_Allgather / MPI_Alltoallv when the program runs on more than one rank. */
typedef struct {
    void *user;
    int (*allgather)(void *user, const void *send, void *recv, uint64_t bytes);
    int (*alltoallv)(void *user, const void *send, const uint64_t *send_bytes, void *recv, const uint64_t *recv_bytes);
} fries_host_collectives;
int fries_hostcomm_create(fries_transport **out, const fries_host_collectives *cb, int rank, int size, int device, uint64_t big_bytes);
/* fills *comm for fries_set_comm; the transport must outlive the context */
int fries_transport_comm(fries_transport *t, fries_comm *comm);
int fries_transport_counts(fries_transport *t, uint64_t *n_allgather, uint64_t *n_alltoallv);
void fries_transport_destroy(fries_transport *t);

/* call between fries_set_molecule and fries_frisys_setup; without it the context is one rank */
int fries_set_comm(fries_ctx *ctx, const fries_comm *comm);
/* the HIP stream (hipStream_t) every kernel of this context is launched on */
void *fries_stream(fries_ctx *ctx);
/* DistVec::idx_to_proc (vec_utils.hpp:360-379) for n determinants; valid after fries_frisys_setup */
int fries_idx_to_proc(fries_ctx *ctx, const uint64_t *dets, size_t n, int32_t *proc);

/* frisys_mol's run parameters (FRIES_bin/frisys_mol.cpp:16-33) plus the seed the reference takes
 * from the wall clock (:104-106). */
typedef struct {
    double epsilon, target_norm, initiator;
    uint32_t vec_nonz, mat_nonz, max_dets;
    uint32_t seed;
    int32_t hb_unnorm;      /* 1: --distribution HB_unnorm, 0: HB */
} fries_frisys_params;

typedef struct {
    double numer, denom;    /* projnum.txt / projden.txt */
    double shift, norm;     /* S.txt / norm.txt */
    uint32_t nkept;         /* nkept.txt */
    int32_t n_nonz;
    uint32_t curr_size;
    uint32_t num_success;   /* comp_vecs.vec_len after apply_HBPP_sys */
    uint32_t comp_len[5];
    uint32_t err;
} fries_iter_log;

/* Optional inputs of the frisys_mol and fciqmc_mol drivers, each before fries_frisys_setup / fries_fciqmc_setup (for fciqmc_mol the
 * initial values are walker numbers, and the last entry of the trial file counts twice in the trial vector, as in the
 * reference's `while (!add) perform_add` loop, fciqmc_mol.cpp:163-170; fciqmc_fp_mol, real_walkers = 1, keeps the initial values real,
 * fciqmc_fp_mol.cpp:157-185, 233-246; fries_frimulti_setup takes --ini_vec with real values, frimulti_mol.cpp:205-215, and answers a trial vector with the
 * reference's own error "Insufficient memory allocated in adder", frimulti_mol.cpp:149-157, which that driver raises for every trial file):
 *   --trial_vec (frisys_mol.cpp:157-181): the vector the energy is projected on, entries add()ed in the given order;
 *   --ini_vec   (:264-274): the starting vector instead of 100 x HF, entries add()ed in the given order (from rank 0);
 *   --ham_shift (:95-98): the offset subtracted from every diagonal element instead of the HF energy (pass ham_shift - core_en). */
int fries_set_trial_vector(fries_ctx *ctx, const uint64_t *dets, const double *vals, size_t n);
int fries_set_initial_vector(fries_ctx *ctx, const uint64_t *dets, const double *vals, size_t n);
int fries_set_ham_shift(fries_ctx *ctx, double hf_en);
/* --det_space (frisys_mol.cpp:236-239, 347-401, 480-485; DistVec::init_dense, vec_utils.hpp:858-897): the determinants of the semi-stochastic
 * dense space.  They take positions 0 .. n - 1 of the vector, are never compressed or deleted, H restricted to them is applied exactly every
 * iteration, and the matrix compression gets mat_nonz minus the number of (symmetry-allowed) matrix elements inside the space.  Before
 * fries_frisys_setup.  With ranks: pass the whole list on every rank; each keeps the determinants it owns, in list order. */
int fries_set_det_space(fries_ctx *ctx, const uint64_t *dets, size_t n);
/* frisys_mol.cpp:76-346: scramblers, solution vector, HF trial vector and H*trial, p_doub, HF start.
 * With ranks: vec_nonz / mat_nonz / target_norm are the GLOBAL budgets, max_dets is per rank, and every rank
 * must pass the same seed (the reference broadcasts rank 0's scramblers and uniforms). */
int fries_frisys_setup(fries_ctx *ctx, const fries_frisys_params *p);
/* frisys_mol.cpp:405-552, n_iter times; logs may be NULL or hold n_iter entries */
int fries_frisys_iterate(fries_ctx *ctx, uint32_t n_iter, fries_iter_log *logs);
double fries_p_doub(fries_ctx *ctx);
/* the proc / vec hash scramblers drawn at setup (frisys_mol.cpp:132-145; hash.dat holds the first, io_utils.cpp:589-606).
 * Either pointer may be NULL; n = 2 * n_orb entries each. */
int fries_get_scramblers(fries_ctx *ctx, uint32_t *proc_scrambler, uint32_t *vec_scrambler, size_t n);
/* --load_dir: the proc scrambler read from hash.dat (load_proc_hash, io_utils.cpp:608-619; frisys_mol.cpp:128-130) instead of 2 n_orb
 * fresh draws -- the shards of a restarted run must be the shards of the run that wrote the checkpoint.  Before fries_frisys_setup;
 * the setup then draws only the vec scrambler, as the reference does. */
int fries_set_proc_scrambler(fries_ctx *ctx, const uint32_t *proc_scrambler, size_t n);
uint64_t fries_kernel_launches(fries_ctx *ctx);

/* ---- frifull_mol: FRI with the Hamiltonian applied in full (FRIES_bin/frifull_mol.cpp:258-304): systematic compression of
 * the vector to vec_nonz non-zeros, then every symmetry-allowed single and double excitation of every remaining determinant
 * (h_op_diag / h_op_offdiag, FRIES/Hamiltonians/molecule.cpp:205-219, 448-665) merged into the other value column.  HF trial
 * vector, start from 100 x HF, one rank.  Logs: numer / denom as written to projnum.txt / projden.txt (:296-300), norm = the
 * one-norm before compression, num_success = non-zero excitations added; n_nonz / curr_size count stored determinants (an entry
 * is released only when it is zero in both value columns, vec_utils.hpp:458-476, so the table keeps growing as in the
 * reference).  spawn_cap: excitations merged per batch (0 = 8e6). */
typedef struct {
    double epsilon, target_norm;
    uint32_t vec_nonz, max_dets, seed, spawn_cap;
} fries_frifull_params;
int fries_frifull_setup(fries_ctx *ctx, const fries_frifull_params *p);
int fries_frifull_iterate(fries_ctx *ctx, uint32_t n_iter, fries_iter_log *logs);

/* ---- frisys_hh: FRI with systematic matrix compression for the 1-D Hubbard-Holstein model (FRIES_bin/frisys_hh.cpp),
 * open boundaries, hopping t = 1, 3 bits per phonon (:96).  Parameters are those of the reference's params file
 * (parse_hh_input, FRIES/io_utils.cpp:320-405: n_elec, lat_len, eps, U, omega, g, gs_energy) and command line (:15-23),
 * plus the seed.  Index = [alpha sites | beta sites | 3 bits per site] in one uint64_t (FRIES/hh_vec.hpp), n_sites <= 12.
 * Start: 100 x the Neel state (:113-117).  Logs: numer / denom are what projnum.txt / projden.txt receive on the rank that
 * owns the Neel state (:338-347) and 0 elsewhere; num_success = samples after the second compression.
 * Shares the vector accessors, fries_set_comm and fries_frisys_restart with frisys_mol. */
typedef struct {
    uint32_t n_elec, n_sites;
    double eps, U, omega, g, gs_energy, target_norm, initiator;
    uint32_t vec_nonz, max_dets, seed;
    uint32_t full;      /* 0: frisys_hh.  1: frifull_hh (FRIES_bin/frifull_hh.cpp) -- every hop and phonon move of every stored state
                         * instead of the two matrix compressions; num_success = number of adds; over ranks as long as a shard's adds of one
                         * iteration fit one Adder (200 000), as the reference ships them in one round then */
} fries_hh_params;
int fries_hh_setup(fries_ctx *ctx, const fries_hh_params *p);
int fries_hh_iterate(fries_ctx *ctx, uint32_t n_iter, fries_iter_log *logs);
/* The same driver's operators one by one, for a host loop that keeps the reference's shape (FRIES_bin/frisys_hh.cpp behind include/FRIES):
 *   fries_set_vec_scrambler   the vector hash's scrambler (the reference's table compares a truncated index inside a bucket chosen by that hash,
 *                             det_hash.hpp:47, so which states share an entry depends on it); with fries_set_proc_scrambler, before fries_hh_setup;
 *   fries_hh_comp_sub         one of the two comp_sub calls (:187-224): stage 1 on the magnitudes of the stored vector with the rows (t, g),
 *                             stage 2 on stage 1's emissions with their uniform subdivisions; outputs as comp_idx[k][0..1] and the value array;
 *   fries_hh_ref_ovlp         calc_ref_ovlp of this rank's shard against the Neel state (hub_holstein.hpp:93-186);
 * the vector itself goes through fries_vec_load / fries_vec_add_to / fries_vec_add_vecs / fries_find_preserve / fries_sys_comp. */
int fries_set_vec_scrambler(fries_ctx *ctx, const uint32_t *vec_scrambler, size_t n);
int fries_hh_comp_sub(fries_ctx *ctx, int stage, uint32_t n_samp, double rn, uint32_t *idx0, uint32_t *idx1, double *vals, size_t cap, size_t *n_out);
int fries_hh_ref_ovlp(fries_ctx *ctx, double *ovlp);

/* ---- fciqmc_mol: FCIQMC with the near-uniform or the heat-bath excitation generator (FRIES_bin/fciqmc_mol.cpp), HF trial
 * vector, start from 100 walkers on HF; one rank or hash-sharded ranks (fries_set_comm: one all-to-all of the spawns per
 * iteration; n_nonz / n_ini in the log are this rank's, norm and the projections global).  The reference's sequential mt19937
 * stream cannot be replayed in parallel;
 * the engine draws from a counter-based stream keyed by (seed, iteration, determinant, attempt, purpose) -- the same uniforms
 * in distribution -- which the CPU oracle shares, and the oracle's functions and loop are pinned against the reference on the
 * reference's own stream (oracle/ref_harness.cpp: fciqmc).  Walker numbers are exact integers in the vector's doubles. */
typedef struct {
    double epsilon;
    uint32_t target_walkers, initiator, max_dets, seed;
    int32_t heat_bath;          /* 0: --distribution NU (near_uniform.cpp), 1: --distribution HB (hb_doub_multi, heat_bathPP.cpp:601-683) */
    int32_t real_walkers;       /* 0: fciqmc_mol.  1: fciqmc_fp_mol (FRIES_bin/fciqmc_fp_mol.cpp): real-valued walkers -- |v| rounded stochastically to
                                 * the number of attempts (:342), spawns below 0.01 rounded and kept real otherwise (:385-390), death in place (:423-424),
                                 * then every |v| < 1 rounded to -1 / 0 / 1 and zeros deleted (:428-441); ranks as for fciqmc_mol (incl. the
                                 * gather at :461-462 that overwrites rank 0's projection terms with the HF owner's); no text vectors */
} fries_fciqmc_params;
typedef struct {
    double numer, denom;        /* projnum.txt / projden.txt */
    double shift, norm;         /* S.txt; walkers at the last shift update (N.txt), 0 on other iterations */
    int32_t n_nonz;             /* nnonz.txt */
    uint32_t n_ini;             /* nini.txt */
    uint32_t curr_size, n_spawn, n_attempts, err;
} fries_fciqmc_log;
int fries_fciqmc_setup(fries_ctx *ctx, const fries_fciqmc_params *p);
int fries_fciqmc_iterate(fries_ctx *ctx, uint32_t n_iter, fries_fciqmc_log *logs);

/* ---- frimulti_mol: FRI with multinomial matrix compression (FRIES_bin/frimulti_mol.cpp), --distribution HB (the only one the
 * reference's argument check lets through, :38-46): every iteration one systematic comb over |v| gives each column its number of
 * samples (:301-322), the samples are drawn with hb_doub_multi / sing_multin and spawn real-valued weights (:343-376), the
 * diagonal acts in place (:379-380), and the vector is compressed to vec_nonz by find_preserve + sys_comp (:385-421).  The first ten
 * iterations use mat_nonz / 10 samples (:306).  Random numbers as for fciqmc_mol: the two comb offsets per iteration come from the
 * mt19937, the sampling from the counter-based stream shared with the CPU oracle, whose loop is pinned against the reference on the
 * reference's stream (oracle/ref_harness.cpp: frimulti).  One rank or hash-sharded ranks (fries_set_comm).  Log: norm = one-norm before the compression (norm.txt),
 * n_nonz / curr_size after it, n_spawn = adds, n_attempts = samples. */
typedef struct {
    double epsilon, target_norm, initiator;
    uint32_t vec_nonz, mat_nonz, max_dets, seed;
} fries_frimulti_params;
int fries_frimulti_setup(fries_ctx *ctx, const fries_frimulti_params *p);
int fries_frimulti_iterate(fries_ctx *ctx, uint32_t n_iter, fries_fciqmc_log *logs);

/* DistVec accessors (FRIES/vec_utils.hpp:506-535): positions [0, curr_size) incl. holes (value 0) */
int fries_vec_info(fries_ctx *ctx, uint32_t *curr_size, int32_t *n_nonz, uint32_t *n_free);
int fries_vec_download(fries_ctx *ctx, uint64_t *dets, double *vals, size_t cap, size_t *n);
/* DistVec::add + perform_add(0) into column 0 with one rank (vec_utils.hpp:418-440, 606-641) */
int fries_vec_add(fries_ctx *ctx, const uint64_t *dets, const double *vals, const uint8_t *ini, size_t n);
/* the same with curr_vec_idx = column (0 or 1): column 1 collects the spawns under the initiator rule (frisys_mol.cpp:424-471).
 * With ranks the list is what THIS rank received (DistVec::add_elements, vec_utils.hpp:606-641): the caller has routed the adds
 * (MPI_Alltoallv inside Adder::perform_add) and passes them in arrival order; nothing is exchanged here. */
int fries_vec_add_to(fries_ctx *ctx, int column, const uint64_t *dets, const double *vals, const uint8_t *ini, size_t n);
/* frisys_mol.cpp:487-499: death / cloning of the first vec_size positions, add_vecs(0, 1), zero_vec on column 1 */
int fries_death_clone(fries_ctx *ctx, double eps, double shift, uint32_t vec_size);
/* DistVec::dot with H * trial (numer) and the trial vector (denom) (frisys_mol.cpp:511-517) */
int fries_dots(fries_ctx *ctx, double *numer, double *denom);
/* find_preserve (compress_utils.cpp:29-105) and sys_comp (:283-327) as two calls, as in the drivers' loops; the preserved
 * set lives on the device in between; fries_sys_comp ends with the deletes of frisys_mol.cpp:534-539 */
int fries_find_preserve(fries_ctx *ctx, uint32_t *n_samp, double *glob_norm);
int fries_sys_comp(fries_ctx *ctx, uint32_t n_samp, double rn);
/* replaces the stored vector: determinants land in positions 0..n-1 (DistVec::load, vec_utils.hpp:761-844) */
int fries_vec_load(fries_ctx *ctx, const uint64_t *dets, const double *vals, size_t n);
/* A checkpoint that holds a dense (semi-stochastic) space (DistVec::load returns n_dense_, vec_utils.hpp:766-779, 844; frisys_mol.cpp:257-263,
 * 347-401): after fries_vec_load, the first n_dense positions become this rank's dense space -- kept whatever their value, H inside the
 * space tabulated again, the matrix sample budget reduced by the number of its elements over all ranks.  Collective with ranks.
 * fries_dense_sizes: every rank's n_dense, what DistVec::save writes to dense.txt (:736-745). */
int fries_vec_set_dense(fries_ctx *ctx, uint32_t n_dense);
int fries_dense_sizes(fries_ctx *ctx, uint32_t *sizes, size_t cap, size_t *n_ranks);
/* Column mirrors for hosts that keep the reference's pointer semantics (DistVec::values(), operator[], zero_vec, matr_el_at_pos,
 * dot: vec_utils.hpp:506-508, 647-649, 577-579, 672-677, 228-238) -- what include/FRIES/vec_utils.hpp is built on.
 * fries_vec_dot_list sums in list order, bit-identical to the reference's loop. */
int fries_vec_column_download(fries_ctx *ctx, int column, double *out, size_t cap, size_t *n);
int fries_vec_column_upload(fries_ctx *ctx, int column, const double *in, size_t n);
int fries_vec_column_zero(fries_ctx *ctx, int column);
/* DistVec::add_vecs(idx1, idx2, c) (vec_utils.hpp:553-557) */
int fries_vec_add_vecs(fries_ctx *ctx, int idx1, int idx2, double c);
int fries_vec_diag_download(fries_ctx *ctx, double *out, size_t cap, size_t *n);
int fries_vec_dot_list(fries_ctx *ctx, int column, const uint64_t *dets, const double *vals, size_t n, double *out);
int fries_htrial_download(fries_ctx *ctx, uint64_t *dets, double *vals, size_t cap, size_t *n);
/* Time-reversal symmetry: vectors that hold one representative of every pair {determinant, its spin-flipped image} (the spin_parity = +-1
 * argument of the reference's h_op_offdiag and apply_HBPP_piv, FRIES/Hamiltonians/molecule.cpp:298-369, 472-552, heat_bathPP.cpp:1326-1407;
 * flip_spins, FRIES/fci_utils.c:158-204).  fries_set_spin_parity(ctx, +-1) makes every full enumeration of H on this context (H * trial at
 * setup, fries_frifull_iterate, the dense block of --det_space, fries_h_offdiag_list) and fries_apply_hbpp_piv (unnormalised heat bath
 * only, as in the reference) form the elements between the symmetrised functions; 0 switches it off.
 * fries_h_offdiag_list: h_op_offdiag(vec, dest_idx 1, h_fac 1, spin_parity) on a fresh two-column vector holding the list in column 0
 * (molecule.cpp:448-665): the stored determinants in position order with column 1. */
int fries_set_spin_parity(fries_ctx *ctx, int spin_parity);
int fries_h_offdiag_list(fries_ctx *ctx, const uint64_t *dets, const double *vals, size_t n, uint64_t *out_dets, double *out_vals, size_t cap, size_t *n_out);
/* The replica estimator: <a|H|b> and <a|b> between column 0 of two contexts' solution vectors -- calc_h_dot (FRIES/Hamiltonians/molecule.cpp:667-885:
 * enumerate H from one vector's columns, look the targets up in the other, add the diagonal) and DistVec::internal_dot for the overlap, as
 * obs_repl_mol uses them on independent replicas.  h / ovlp needs no trial vector; with a == b (allowed) it is the Rayleigh quotient of the vector.
 *   ovlp    = sum_i a_i b_i
 *   h       = sum_i a_i d_i b_i + sum_i sum_{j in exc(i)} a_i m_ij b_j
 *   abs_sum = the same sum as h over the magnitudes of its terms (a bound for h's rounding error: ~(n_hits + n_src) * 2^-53 * abs_sum)
 * i runs over the stored determinants of `a` with a non-zero value; d_i is the diagonal element minus the offset of the run (the HF
 * energy, or what fries_set_ham_shift set), so h / ovlp is on the scale of numer / denom; exc(i) and m_ij are the symmetry-allowed singles
 * and doubles and their signed elements exactly as fries_h_offdiag_list enumerates them, fries_set_spin_parity included; b_j is looked up in
 * b's hash table.  n_src = sources visited, n_terms = excitations with a non-zero element, n_hits = those found in b with a non-zero
 * value.  `a` is the enumerating side: pass the shorter vector there.  Deterministic: no floating-point atomics, two calls on the
 * same vectors return the same bits.  Nothing of either vector is changed and nothing stays allocated.
 * Ordering and threads: the kernels run on a's stream after everything b's stream holds at the time of the call, and the call
 * returns when the result is on the host.  Neither context may be inside another call on another thread while this one runs.
 * Refused with a message and without a launch: a context without a molecule and a solution vector, a Hubbard-Holstein context, a
 * context with a communicator, contexts on different devices, or contexts that differ in n_orb, n_elec, irreps, hf_en or spin_parity.
 * Over ranks: fries_h_dot_ranks below, against a fries_snapshot of the probed side (this call keeps refusing a context with a communicator).
 * Out of scope: more than one value column per side, Hubbard-Holstein,
 * replicas for drivers other than frisys_mol_hip, and a binding in include/FRIES (that facade holds one device-bound vector per
 * process).  fries_frisys_iterate, its launch count and its draws are untouched. */
typedef struct { double h, ovlp, abs_sum; uint64_t n_src, n_terms, n_hits; } fries_hdot_result;
int fries_h_dot(fries_ctx *a, fries_ctx *b, fries_hdot_result *out);
/* The one-body density matrix between two replicas: gamma[p * n_orb + q] = <a| sum_sigma c+_{p sigma} c_{q sigma} |b> over column 0 of the two
 * contexts' solution vectors, all n_orb * n_orb orbital pairs in one pass.  For p != q it is what the reference forms for ONE pair per run
 * -- one_elec_op(vec, n_orb, des = q, cre = p, 2) (FRIES/Hamiltonians/molecule.cpp:222-252) with column 0 holding b and column 1 holding a,
 * then DistVec::internal_dot(1, 2), as observables_mol and obs_repl_mol do: the sum over both spins of a_i * sign * b_j, where |i> is |j>
 * with spin orbital q sigma emptied and p sigma filled and sign = (-1)^(occupied spin orbitals strictly between them) (sing_det_parity).
 * The diagonal is the number operator, gamma[p][p] = sum_i a_i b_i (n_{p alpha}(i) + n_{p beta}(i)): one_elec_op itself yields nothing for
 * des == cre (its test read_bit(des) && !read_bit(cre) cannot hold), and the occupation is the meaningful diagonal.  Hence
 * trace(gamma) = n_elec * <a|b>, gamma(a, b)[p][q] = gamma(b, a)[q][p], and every one-electron expectation value is sum(op * gamma) / ovlp.
 *   ovlp    = <a|b> = sum_i a_i b_i
 *   abs_sum = the sum of the magnitudes of all off-diagonal terms
 *   n_src   = stored determinants of `a` with a non-zero value; n_terms = probes issued = n_src * n_elec * (n_orb - n_elec / 2);
 *   n_hits  = probes that found a non-zero value in b
 * No symmetry is consulted: a bin whose orbitals differ in irrep is the sum of whatever the vectors hold.
 * As in fries_h_dot: `a` enumerates and `b` is only probed (pass the shorter vector as `a` and transpose); neither vector, diagonal cache
 * nor host mirror changes; a == b is allowed; the kernels run on a's stream after everything b's stream holds at the time of the call, the
 * call returns when the result is on the host, and neither context may be inside another call on another thread meanwhile.  Deterministic:
 * no floating-point atomics, two calls on the same vectors return the same bits in every bin.  Nothing stays allocated.
 * Refused with a message and without a launch: a null argument, a context without a molecule or without a solution vector, a
 * Hubbard-Holstein context, a context with a communicator, contexts on different devices or that differ in n_orb, n_elec or irreps, and
 * spin_parity != 0 on either side (a time-reversal vector stores one representative per pair).  hf_en plays no part and is not compared.
 * Over ranks: fries_rdm1_ranks below.  Out of scope: time-reversal vectors, Hubbard-Holstein, the importance-weighted
 * compression of observables_mol (weight_vec, --exponent), a binding in include/FRIES, and replicas for drivers other than frisys_mol_hip. */
typedef struct { double ovlp, abs_sum; uint64_t n_src, n_terms, n_hits; } fries_rdm1_result;
int fries_rdm1(fries_ctx *a, fries_ctx *b, double *gamma /* n_orb * n_orb, row-major */, fries_rdm1_result *out);
/* The two-body density matrix between two replicas, spin-summed and in chemists' order, over column 0 of the two contexts' solution vectors:
 *   gamma2[((p * n_orb + q) * n_orb + r) * n_orb + s] = sum over sigma, tau of <a| c+_{p sigma} c+_{r tau} c_{s tau} c_{q sigma} |b>
 * Bit p of a determinant is orbital p with spin alpha, bit p + n_orb orbital p with spin beta; every operator's sign is the parity of the
 * occupied bits below it at its turn.  Three kinds of pairs (i, j) contribute a_i * sign * b_j: i == j (the diagonal: every ordered pair
 * of occupied spin orbitals P != R gives +1 to [p][p][r][r] and, with equal spins, -1 to [p][r][r][p]), pairs one same-spin replacement
 * apart (the replacement times every spectator, direct and same-spin exchange) and pairs two replacements apart (the two direct and the
 * two exchange pairings, each where its spins match).  With gamma of fries_rdm1 and (pq|rs) the molecule's integrals:
 *   sum_pq h_pq gamma[p][q] + 1/2 sum_pqrs (pq|rs) gamma2[p][q][r][s] = <a|H|b>    (fries_h_dot's h + hf_energy * ovlp)
 *   sum_r gamma2[p][q][r][r] = (n_elec - 1) gamma[p][q];   sum_pr gamma2[p][p][r][r] = n_elec (n_elec - 1) <a|b>
 *   gamma2[p][q][r][s] == gamma2[r][s][p][q] bit for bit;   gamma2(a, b)[p][q][r][s] = gamma2(b, a)[q][p][s][r]
 *   <S^2> = -N (N - 4) / 4 - 1/2 sum_pq gamma2[p][q][q][p] / ovlp
 *   ovlp    = <a|b>;  abs_sum = the sum of |a_i b_j| over the hits, once per hit
 *   n_src   = stored determinants of `a` with a non-zero value;  n_hits = probes that found a non-zero value in b
 *   n_terms = probes issued: per source its 2 h (n - h) singles, 2 C(h,2) C(n-h,2) same-spin and h^2 (n - h)^2 opposite-spin doubles
 *             (h = electrons per spin, n = n_orb; counted from the determinant's own occupation)
 * No symmetry is consulted: a bin whose four irreps do not multiply to the identity is the sum of whatever the vectors hold.
 * As in fries_rdm1: `a` enumerates and `b` is only probed (pass the shorter vector as `a` and use the adjoint relation); neither vector,
 * diagonal cache nor host mirror changes; a == b is allowed; the kernels run on a's stream after everything b's stream holds at the time of
 * the call, the call returns when the result is on the host, and neither context may be inside another call on another thread meanwhile.
 * Deterministic: no floating-point atomics; a counting pass sizes the bin records, the positions are cut into chunks of at most
 * FRIES_RDM2_RECORDS records (read when `a` is created; default 2^25, 24 bytes each), each chunk is sorted by bin with a stable sort and
 * added in order.  Two calls on the same vectors with the same capacity return the same bits.  Nothing stays allocated.
 * Refused with a message and before the first launch: a null argument, a context without a molecule or without a solution vector, a
 * Hubbard-Holstein context, a context with a communicator, contexts on different devices or that differ in n_orb, n_elec or irreps, and
 * spin_parity != 0 on either side.  hf_en is not compared.  Refused after the counting pass, before any record is written: 32 positions
 * whose records exceed the capacity, and scratch that exceeds the free device memory.
 * Over ranks: fries_rdm2_ranks below.  Out of scope: time-reversal vectors, Hubbard-Holstein, three-body quantities, the importance-weighted compression of
 * observables_mol, a binding in include/FRIES, replicas for other drivers, and skipping probes by point-group symmetry. */
typedef struct { double ovlp, abs_sum; uint64_t n_src, n_terms, n_hits; } fries_rdm2_result;
int fries_rdm2(fries_ctx *a, fries_ctx *b, double *gamma2 /* n_orb^4, row-major */, fries_rdm2_result *out);

/* ---- Vector snapshots, and the three estimators over ranks.
 * A snapshot is an immutable, device-resident copy of column 0 of a solution vector, sharded over ranks or not: the shards' live
 * entries (value != 0) as one (determinant, value) list -- every shard's entries in position order, the shards in rank order, so the
 * content is a function of the vectors alone -- and one open-addressed look-up table over the list (16-byte slots, linear probing, at
 * most 40 % full, at least 2^14 slots: the layout and the hash of the vector's own table).  It is what the probed side `b` of
 * fries_h_dot, fries_rdm1 and fries_rdm2 needs and nothing more: those kernels read b's table and b's values only.  A snapshot outlives
 * whatever its source does next (iterate it, destroy it): it is built once per meeting of the replicas and serves all three estimators
 * and every partner that probes that replica.
 * fries_snapshot_create: a stable compaction on every shard's own stream, a copy of the lists to `device` (hipMemcpyPeerAsync; an
 * ordinary copy where the devices are equal), one insert kernel there (64-bit compare-and-swap on the key, plain store of the
 * position).  The call returns after a synchronisation: nothing reads the table before, and later users need no cross-stream wait.
 * All device memory is sized from the shards' curr_size and checked against the free memory of every device involved before
 * anything is allocated or launched; the staging is freed before the call returns, the rest belongs to the snapshot until
 * fries_snapshot_destroy (a null snapshot is left alone).  The shards are only read.
 * Refused with a message that names fries_snapshot_create and without a launch: a null argument; n_shards of 0 or above 64; a
 * Hubbard-Holstein context; a context without a molecule or without a solution vector; shards that are not exactly ranks
 * 0 .. n_shards - 1 of one run, in order (a context's communicator has another size than n_shards, entry k is not rank k, or the
 * contexts' rank scramblers or iteration counts differ: what determines a run's content -- a context without a communicator is the
 * one shard of a run of one); shards that differ in n_orb,
 * n_elec, irreps, hf_en or spin_parity; a device index out of range; more than 2^32 - 2 positions.  Refused after the insert: a
 * determinant that two shards hold or that is no valid key, a full table.
 * Threads: one host thread makes the call, and no context among the shards may be inside another call meanwhile.  The calls of this
 * section select devices of their own and put the calling thread's current device back before they return.
 * The fill follows FRIES_HASH_FILL where it is set, as the vector's own table does (default 40).
 * fries_snapshot_info: n_entries, the number of shards, the table's slots, the device bytes the snapshot owns, its device, and -- only
 * where FRIES_SNAPSHOT_EVENTS=1 was set when the library first built a snapshot, otherwise 0 -- what the three steps of the build took on
 * the device (HIP events; the compaction summed over the shards' streams).
 * fries_snapshot_vector: the entries in the snapshot's order (rank-major, position order within a rank); *n = n_entries even when cap is
 * too small (the call then fails); dets or vals may be NULL. */
typedef struct fries_snapshot fries_snapshot;
typedef struct { uint64_t n_entries; uint32_t n_shards, n_slots; uint64_t device_bytes; int32_t device; float ms_compact, ms_copy, ms_insert; } fries_snapshot_info_t;
int fries_snapshot_create(fries_snapshot **s, fries_ctx *const *shards, uint32_t n_shards, int device);
int fries_snapshot_info(const fries_snapshot *s, fries_snapshot_info_t *out);
int fries_snapshot_vector(const fries_snapshot *s, uint64_t *dets, double *vals, uint64_t cap, uint64_t *n);
int fries_snapshot_destroy(fries_snapshot *s);
/* fries_h_dot, fries_rdm1 and fries_rdm2 with the enumerating side `a` given as the n_a shards of one run and the probed side `b` as a
 * snapshot: the unchanged kernels of the two-context calls run once per shard of `a`, on that shard's stream, against the snapshot's
 * table, one shard after the other (an empty shard launches nothing), and the shards' results are added on the host in rank order --
 * the scalars and the counts, every bin of gamma, every bin of gamma2 after each shard's own symmetrisation, so that
 * gamma2[p][q][r][s] == gamma2[r][s][p][q] stays bit for bit.  The results are those of the two-context calls on the unions of the
 * shards up to the association order of the sums: the counts are equal, and with one shard per side every bit is.  Deterministic: two
 * calls on the same shards and snapshot return the same bits.  `a` is only read; a snapshot of `a` itself may be passed as `b`.
 * Refused with a message that names the entry point and before the first launch: a null argument; `a` failing the completeness rule of
 * fries_snapshot_create; a shard of `a` on another device than the snapshot; another molecule than the snapshot's (n_orb, n_elec,
 * irreps); for fries_h_dot_ranks a differing hf_en or spin_parity; for the density matrices spin_parity != 0 on either side or more
 * than 32 orbitals.  What a shard's positions need in bin records is known only after its counting pass, as in fries_rdm2: fries_rdm2_ranks
 * runs every shard's counting pass (one launch per non-empty shard) and refuses a capacity (FRIES_RDM2_RECORDS) below any workgroup's need,
 * naming the shard, before a single record is written; gamma2 and *out are then left zero.  The scratch of a shard's records is checked
 * against the free memory when that shard's turn comes.
 * Threads: one host thread makes the call; no context of `a` may be inside another call on another thread meanwhile, and the snapshot
 * must not be destroyed.  Several threads may probe one snapshot at the same time with different `a`.
 * Out of scope: ranks in separate processes (a snapshot needs all shards in one process), frisys_mol_hip --replicas with --ranks,
 * time-reversal vectors in the density matrices, Hubbard-Holstein, the other drivers.  No run on more than one GPU has been made. */
int fries_h_dot_ranks(fries_ctx *const *a, uint32_t n_a, const fries_snapshot *b, fries_hdot_result *out);
int fries_rdm1_ranks(fries_ctx *const *a, uint32_t n_a, const fries_snapshot *b, double *gamma /* n_orb * n_orb */, fries_rdm1_result *out);
int fries_rdm2_ranks(fries_ctx *const *a, uint32_t n_a, const fries_snapshot *b, double *gamma2 /* n_orb^4 */, fries_rdm2_result *out);

/* ---- what a loop over several vectors needs beside the operators below (fries_amd/subspace.py: the reference's subsp_mol loop with one
 * context per state): the one step that mixes vectors, a plain overlap, a scale and a one-norm.
 * Each of the four refuses with a message that names it and before the first launch: a null argument; a Hubbard-Holstein context; a
 * context without a molecule or without a solution vector; a column other than 0 or 1; a snapshot on another device than the context; a
 * snapshot of another molecule (n_orb, n_elec, irreps) or spin_parity.
 *
 * fries_vec_axpy_snapshot: column[det] += coeff * x[det] for every entry of the snapshot that this context owns -- all of them without
 * a communicator, those with idx_to_proc(det) == rank with one.  The whole snapshot is on the device, so the call is no collective and
 * needs no exchange: every rank takes its own.  The product is rounded once, fl(coeff * x); an entry whose product is 0 is dropped, as
 * DistVec::add drops zero values.  The rest are merged in the snapshot's order with initiator flag 1, as fries_vec_add_to merges a host
 * list: a determinant not yet stored gets the position that call would give it, and a vector whose capacity (max_dets) the inserts
 * would exceed is refused as there.  The owned entries are staged into the context's spawn buffers on the device (count, scan, write:
 * nothing passes through the host), in chunks of at most the spawn capacity, one merge per chunk, in list order.  coeff == 0 or an empty
 * snapshot returns at once without a launch.  *n_taken = the entries merged.  A pending compression result is cleared, as by any merge. */
int fries_vec_axpy_snapshot(fries_ctx *ctx, int column, double coeff, const fries_snapshot *x, uint64_t *n_taken);
/* fries_snapshot_dot: sum_i a_i * b(det_i) over the stored positions of the shards of `a` with a non-zero value in `column`, each looked
 * up in the snapshot's table.  `a` follows the completeness rule of fries_snapshot_create.  One pass per shard on that shard's stream
 * (an empty shard launches nothing); the shards are added on the host in rank order.  abs_sum = the sum of the magnitudes of the
 * products, n_src = the positions with a non-zero value, n_hits = those found in the snapshot with a non-zero value.  No floating-point
 * atomics: per-wave sums in a fixed order, one partial per 1024-position tile, the partials added in tile order; two calls on the same
 * data return the same bits. */
typedef struct { double dot, abs_sum; uint64_t n_src, n_hits; } fries_vdot_result;
int fries_snapshot_dot(fries_ctx *const *a, uint32_t n_a, int column, const fries_snapshot *b, fries_vdot_result *out);
/* v[column][i] *= factor over the stored positions */
int fries_vec_scale(fries_ctx *ctx, int column, double factor);
/* DistVec::local_norm + sum_mpi: the sum of |v[column][i]| in position order, then over the ranks in rank order.  With a communicator a
 * collective (one all-gather). */
int fries_vec_one_norm(fries_ctx *ctx, int column, double *norm);

/* The hot-path operators one by one, on the context's solution vector. */
/* apply_HBPP_sys (heat_bathPP.cpp:686-992) with the five uniforms it would draw; outputs as
 * comp_vecs.{det_indices2, orb_indices1, vec1}.  unit_matrel != 0 uses the |value| = 1 lambdas of
 * tests/test_hamiltonian.cpp:493-500.  det_pos / orbs / vals may each be NULL: the result then stays on the device only
 * (where fries_spawn_from_comp consumes it and fries_comp_download fetches it later); cap must still be >= *n_out. */
int fries_apply_hbpp_sys(fries_ctx *ctx, uint32_t n_samp, const double rn[5], int unit_matrel,
                         uint32_t *det_pos, uint8_t *orbs, double *vals, size_t cap, size_t *n_out, uint32_t comp_len[5]);
/* apply_HBPP_piv (heat_bathPP.cpp:1014-1419; spin_parity = what fries_set_spin_parity set): every factor multiplied out into the long vector, compressed by
 * piv_comp_parallel to n_samp elements and collapsed; outputs as comp_scratch->{det_indices2, orb_indices1, vec1}.  The uniforms
 * come from the context's generator in the reference's order (seed it with fries_frisys_restart), because their number
 * depends on the data.  stage_len[k] = elements after the k-th compression.  One factor may expand to at most 134e6 values. */
int fries_apply_hbpp_piv(fries_ctx *ctx, uint32_t n_samp, int unit_matrel,
                         uint32_t *det_pos, uint8_t *orbs, double *vals, size_t cap, size_t *n_out, uint32_t stage_len[5]);
/* ---- one FRI iteration of frisys_mol step by step, for a host that keeps its own loop: fries_apply_hbpp_sys (no download), the
 * calls below, fries_death_clone, fries_dots, fries_find_preserve, fries_sys_comp.  Nothing larger than a few scalars crosses PCIe.
 *
 * fries_spawn_from_comp: frisys_mol.cpp:429-471.  Consumes the result the last fries_apply_hbpp_sys or fries_apply_hbpp_piv of this
 * context left on the device: forms the spawns -eps * value * sign(origin) on the excited determinants (doub_det / sing_det) and adds
 * them into column 1 in the reference's order -- non-initiator origins first, then initiators, |origin| >= init_thresh judged against
 * column 0 -- as the two add passes + perform_add do.  With a communicator it is a collective: the exchange and the Adder rounds of
 * fries_frisys_iterate (FRIES_ADDER_SIZE included); every rank enters it, also with nothing to send.  Column 1 must be zero on entry
 * (as after setup and after fries_death_clone).  eps and init_thresh are the arguments, not the setup parameters.
 * A compression result refers to positions of the vector as it stood: the context records that one is pending, and whatever changes the
 * layout -- a merge (fries_vec_add*, this call), fries_sys_comp, fries_compress_vec*, fries_vec_load, the setup -- clears the record.
 * With nothing pending the call returns -1 with a message and launches nothing. */
int fries_spawn_from_comp(fries_ctx *ctx, double eps, double init_thresh);
/* frisys_mol.cpp:480-485: the tabulated dense block of H (times -epsilon of fries_frisys_setup, as :347-397 tabulate it) times column 0,
 * added into column 1 as a perform_add of its own.  Collective
 * whenever the dense space is non-empty on any rank; returns 0 at once when there is no dense space. */
int fries_dense_apply(fries_ctx *ctx);
/* sol_vec.dense_norm() of frisys_mol.cpp:504 (vec_utils.hpp:903-918): summed in position order on the device, then over the ranks in
 * rank order (collective with a dense space); 0 without one. */
int fries_dense_norm(fries_ctx *ctx, double *norm);
/* tot_dense_h (frisys_mol.cpp:399): the matrix elements inside the dense space over all ranks; the sample budget of :421 is
 * mat_nonz - tot_dense_h. */
int fries_dense_h_count(fries_ctx *ctx, uint32_t *global_count);
/* the pending compression result, fetched after the fact (comp_vecs.{det_indices2, orb_indices1, vec1} of heat_bathPP.cpp:686-992);
 * any pointer may be NULL; -1 when nothing is pending.  Does not consume the result. */
int fries_comp_download(fries_ctx *ctx, uint32_t *det_pos, uint8_t *orbs, double *vals, size_t cap, size_t *n_out);

/* find_preserve + sys_comp on column 0 (compress_utils.cpp:29-105, 283-327) followed by the deletes
 * of frisys_mol.cpp:534-539 */
int fries_compress_vec(fries_ctx *ctx, uint32_t n_samp, double rn, uint32_t *n_kept, double *glob_norm);

/* compress_vecs with one vector (FRIES/vec_utils.cpp:9-32): piv_comp_parallel on column 0 -- find_preserve,
 * piv_budget, adjust_probs, piv_samp_serial (compress_utils.cpp:354-681) -- then the deletes.  The uniforms are the
 * context's mt19937 stream (the generator the reference's caller passes in), two per sampling unit.  With ranks: a collective
 * call (two all-gathers); rank 0's generator also serves piv_budget. */
int fries_compress_vec_piv(fries_ctx *ctx, uint32_t n_samp, uint32_t *n_kept, double *glob_norm);
/* how many fries_compress_vec_piv calls were settled by the parallel, certified cut-point search and how many fell back to the
 * sequential one (csrc/pivotal.hip); FRIES_PIV_CHAIN=1 in the environment forces the sequential search */
int fries_piv_stats(fries_ctx *ctx, uint64_t *n_certified, uint64_t *n_fallback);
/* the next raw draw of the context's mt19937 (advances it): lets a caller interleave its own draws as the reference's
 * drivers do, and tests check the generator's position */
uint32_t fries_next_draw(fries_ctx *ctx);
/* the generator in std::mt19937's text form (operator<< / operator>>), so that a caller owning a std::mt19937 as the reference's
 * drivers do (frisys_mol.cpp:104-106) can lend it to fries_apply_hbpp_piv / fries_compress_vec_piv and take it back.
 * get: buf may be NULL to query the size (*need, with the terminator; about 6.9 kB) */
int fries_rng_set_state(fries_ctx *ctx, const char *text);
int fries_rng_get_state(fries_ctx *ctx, char *buf, size_t cap, size_t *need);

/* Restart: re-seed the driver RNG, restore the energy shift / last norm / iteration count -- the part of
 * --load_dir that is not the vector (frisys_mol.cpp:257-263, 284-286); pair with fries_vec_load. */
int fries_frisys_restart(fries_ctx *ctx, uint32_t seed, double en_shift, double last_one_norm, uint32_t iterat);

/* running totals since setup: iterations, successful spawns (num_success), kernel launches,
 * find_keep_sub replays, elements emitted by the five HB-PP stages */
int fries_counters(fries_ctx *ctx, uint64_t *iters, uint64_t *spawns, uint64_t *launches, uint64_t *fks_replays, uint64_t *stage_elems);

/* Tie statistics: how close the run came to a comparison whose outcome floating-point reassociation could change.  While enabled,
 * every find_keep_sub stage (its threshold tests v * w * budget >= norm, compress_utils.cpp:172-241) and every find_preserve round
 * (|v| >= norm / budget, :57-63) records the smallest |a - b| / max(a, b) over all its comparisons; the call returns the minima since
 * the last call (infinity when nothing was recorded) and restarts them.  The device forms those norms as prefix sums, the reference as
 * running sums: a margin far above ~1e-13 means the kept sets are provably the same.  enable: 1 start / keep recording, 0 stop. */
int fries_tie_margins(fries_ctx *ctx, int enable, double *fks_min_rel, double *fp_min_rel);

/* device-to-device copy bandwidth of the context's GPU in GB/s (read + write), `reps` copies of `bytes` on the engine's stream */
int fries_measure_copy_bandwidth(fries_ctx *ctx, size_t bytes, int reps, double *gb_per_s);
/* Per-kernel timing with HIP events recorded on the engine's own stream (off by default). */
int fries_prof_enable(fries_ctx *ctx, int on);
int fries_prof_count(fries_ctx *ctx);
int fries_prof_get(fries_ctx *ctx, int i, char *name, size_t name_cap, double *total_ms, uint64_t *calls);

/* test hook: adjust_probs (compress_utils.cpp:606-681) on column 0 with nothing preserved; flags_out[curr_size] = the
 * elements it pinned to one sampling unit */
int fries_test_piv_adjust(fries_ctx *ctx, uint32_t *n_samp_loc, double exp_nsamp_loc, uint32_t n_samp_tot, double tot_norm,
                          double *new_norm, uint8_t *flags_out);

/* test hook: positions of the first n comb teeth built from (r0, unit) -- see csrc/teeth.hpp */
int fries_test_teeth(fries_ctx *ctx, double r0, double unit, uint32_t n, double *out_pos, const double *query, uint32_t nq, uint32_t *out_below);

/* test hook: bit-exact left-to-right running sums S_i = fl(S_{i-1} + vals[i]) of non-negative
 * doubles, evaluated in parallel -- see csrc/seqsum.hpp */
int fries_test_seqsum(fries_ctx *ctx, const double *vals, uint32_t n, double start, double *out_prefix, double *out_total,
                      uint32_t *n_dirty_tiles, uint32_t *n_dirty_subs);

#ifdef __cplusplus
}
#endif
#endif
