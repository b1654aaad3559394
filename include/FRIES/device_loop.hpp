/*! \file  FRIES/device_loop.hpp -- MI355X build only (no counterpart in the reference): what a frisys_mol-shaped loop written against
 * FRIES/*.hpp calls so that the iteration never moves a column, a compression result or a spawn list over PCIe.
 *
 * The reference's loop reads the compression result on the host, builds the excited determinants there and hands them to
 * DistVec::add / perform_add; through the mirrors of FRIES/vec_utils.hpp that costs a download of the result, an upload of the spawns and a
 * refresh of every column the program takes a pointer to.  The calls below replace those stretches of the loop by single device operators
 * (include/fries_hip.h: fries_spawn_from_comp, fries_dense_apply, fries_death_clone, fries_dense_norm); each line range is the one of
 * FRIES_bin/frisys_mol.cpp it stands for.  All of them go through the vector's before_device_op / after_device_op bookkeeping, so a
 * mirror the program does read later (values(), save()) is refreshed then.  A program that includes this header and calls none of it runs
 * exactly as without it. */
#ifndef FRIES_DEVICE_LOOP_HPP
#define FRIES_DEVICE_LOOP_HPP
#include <FRIES/vec_utils.hpp>
#include <FRIES/Hamiltonians/heat_bathPP.hpp>

namespace fries_hip {
/*! on: apply_HBPP_sys leaves det_indices2 / orb_indices1 / vec1 on the device and fills comp_scratch->vec_len only */
inline void keep_comp_on_device(bool on) { Backend::get().comp_on_device = on; }
/*! the arrays of the last apply_HBPP_sys after all, for a host that wants to look at them (the result must still be pending: before
 * spawn_from_comp); returns the number of elements */
inline size_t comp_download(DeviceVecBase &v, HBCompressSys *comp_scratch) {
    size_t n_out = 0;
    ck(fries_comp_download(v.ctx(), comp_scratch->pos32.data(), (uint8_t *)comp_scratch->orb_indices1, comp_scratch->vec1.data(), comp_scratch->vec1.size(), &n_out));
    for (size_t i = 0; i < n_out; i++) comp_scratch->det_indices2[i] = comp_scratch->pos32[i];
    comp_scratch->vec_len = n_out;
    Backend::get().bytes_to_host += 16 * n_out;
    return n_out;
}
inline void need_bound(DeviceVecBase &v, const char *who) {
    if (!v.bound()) throw std::runtime_error(std::string(who) + ": the vector has not moved to the device yet (move_to_device, or the first apply_HBPP_sys, does that)");
}
/*! moves the solution vector to the device before the loop starts (otherwise the first apply_HBPP_sys does it): mat_nonz is the global
 * matrix sample budget, which sizes the operators' work arrays; eps is the time step -- the device tabulates the dense block of H times
 * -eps when the vector arrives (frisys_mol.cpp:347-397), which is what dense_multiply applies, so a loop with a dense space must name it here */
inline void move_to_device(DeviceVecBase &v, uint32_t mat_nonz, bool new_hb, double eps) {
    Backend::get().loop_eps = eps;
    v.bind(mat_nonz, new_hb);
}
/*! tot_dense_h of frisys_mol.cpp:399 as the device tabulated it when the vector moved there */
inline uint32_t dense_h_count(DeviceVecBase &v) {
    need_bound(v, "dense_h_count");
    uint32_t n = 0;
    ck(fries_dense_h_count(v.ctx(), &n));
    return n;
}
/*! frisys_mol.cpp:429-471: the two add passes over the compression result (non-initiators, then initiators) with their perform_add's,
 * into column 1 under the initiator rule against column 0.  Column 1 must be zero. */
inline void spawn_from_comp(DeviceVecBase &v, double eps, double init_thresh) {
    need_bound(v, "spawn_from_comp");
    v.before_device_op();
    ck(fries_spawn_from_comp(v.ctx(), eps, init_thresh));
    v.after_device_op(false, true, true);
}
/*! frisys_mol.cpp:480-485: the dense block of H times column 0, added into column 1 as a perform_add of its own */
inline void dense_multiply(DeviceVecBase &v) {
    need_bound(v, "dense_multiply");
    v.before_device_op();
    ck(fries_dense_apply(v.ctx()));
    v.after_device_op(false, true, true);
}
/*! frisys_mol.cpp:487-499: death / cloning of the first vec_size positions, add_vecs(0, 1), zero_vec on column 1 */
inline void death_clone(DeviceVecBase &v, double eps, double en_shift, size_t vec_size) {
    need_bound(v, "death_clone");
    v.before_device_op();
    ck(fries_death_clone(v.ctx(), eps, en_shift, (uint32_t)vec_size));
    v.after_device_op(true, true, false);
}
/*! sol_vec.dense_norm() of frisys_mol.cpp:504, summed on the device */
inline double dense_norm(DeviceVecBase &v) {
    need_bound(v, "dense_norm");
    v.before_device_op();
    double dn = 0;
    ck(fries_dense_norm(v.ctx(), &dn));
    return dn;
}
/*! what to pass to find_preserve / sys_comp as the value pointer (the reference passes &values()[n_determ]): names the bound vector
 * without refreshing or dirtying its host mirror */
template <class el_type> inline el_type *values_key(const DistVec<el_type> &v) { return v.device_key(); }
/*! what to pass to apply_HBPP_sys as all_dets (the reference passes indices()): the same matrix, its host content left as it is */
template <class el_type> inline Matrix<uint8_t> &indices_key(DistVec<el_type> &v) { return v.device_indices_key(); }
}  // namespace fries_hip
#endif
