/* gmr_amd.h -- C ABI of libgmr_amd.so, the MI355X (gfx950) retarget engine.
 *
 * Plain C: opaque handle, raw pointers, sizes.  No torch / C++ types cross this
 * boundary.  Every pointer documented "device" is a HIP device pointer on the
 * GPU the handle was created for (e.g. torch.Tensor.data_ptr()); "host" pointers
 * are ordinary CPU memory.  The caller owns every buffer; the library owns only
 * the handle (which keeps a copy of the model and a small scheduling workspace).
 * Calls on one handle may be issued on different HIP streams (per-call scheduling
 * data is stream-ordered, nothing is shared between launches); gmr_last_error's
 * buffer is per handle, so concurrent host threads should use one handle each.  All calls return 0 on success and a negative GMR_E* code on
 * failure, with a message available from gmr_last_error().  There is no CPU
 * fallback: without a usable HIP device gmr_model_create fails.
 *
 * Stream order.  An entry that takes a `stream` enqueues all of its work on that stream and on no other: kernels, table copies,
 * memsets, and the allocation and release of its scratch.  Device inputs are read and device outputs written in stream order, so a
 * call may be issued behind the work that produces its inputs and ahead of the work that consumes its outputs with no host
 * synchronisation in between.  Host arrays and structs passed by pointer (slot_col, items, seq_offsets, out_offsets, ratio,
 * parents, out_cols, betas, segment tables, params, the *_input structs and what they point to) are read completely before the
 * call returns and may be reused or freed on return: what the kernels need of them travels as kernel arguments or is copied with
 * hipMemcpyAsync from pageable memory, of which the runtime takes its own copy when it is called.  A call does not wait for the
 * stream: it returns while earlier work on `stream` is still running -- with host tables of up to 512 KiB each (13 000 work
 * items, 65 000 clip offsets).  A larger table (observed at 1 MiB) makes hipMemcpyAsync, and with it the call, wait until the
 * earlier work on `stream` has finished; results and the rule for host arrays are the same.  The entries that synchronise
 * `stream` before they return, because they hand back host data: gmr_bvh_parse_motion_device.  Sessions (gmr_session_*) own
 * their stream and return results to the host.  All of this is checked behind a busy stream for every entry on ROCm 7
 * (tests/test_gpu_stream_order.py).
 *
 * Extent and alignment.  Every device and host array is dense and row-major, of exactly the extent its entry states: there is no
 * padding between rows and none is needed behind the last one.  An array needs only the alignment of its element type (4 bytes
 * for float32 / int32, 8 for float64 / int64, 1 for text bytes; a struct its natural alignment) -- a slice that starts in the
 * middle of a larger allocation is as good as the allocation itself, and no entry asks for more.  Nothing outside the stated
 * extent is read into a result, and nothing outside it is written; inputs are never modified and every element of a non-NULL
 * output is written unless its entry says otherwise.  Checked for every stream-taking entry inside guarded arrays, 256-byte
 * aligned and element-aligned (tests/test_gpu_guard_band.py).
 *
 * What each entry point replaces in the reference (Zudva/GMR):
 *   gmr_model_create   GeneralMotionRetargeting.__init__ + setup_retarget_configuration
 *                      (general_motion_retargeting/motion_retarget.py:13-114): mj.MjModel.from_xml_path,
 *                      mink.Configuration, the two lists of mink.FrameTask;  and
 *                      KinematicsModel.__init__ (kinematics_model.py:69-99)
 *   gmr_ik_solve       the caller loop `for frame in frames: qpos = retargeter.retarget(frame)`
 *                      (scripts/smplx_to_robot_dataset.py:84-89, scripts/bvh_to_robot_dataset.py:95-104)
 *                      i.e. GeneralMotionRetargeting.retarget / update_targets / error1 / error2
 *                      (motion_retarget.py:117-200) and, inside it, mink.solve_ik +
 *                      Configuration.integrate_inplace (call sites motion_retarget.py:147-150,156-159,
 *                      166-169,176-179)
 *   gmr_group_*        several robots' batches in one launch (one GeneralMotionRetargeting per robot in the reference)
 *   gmr_session_*      the live loop of scripts/optitrack_to_robot.py:37-46 / smplx_to_robot.py:103-126 / bvh_to_robot.py:
 *                      one frame in, one qpos out, state carried inside (`retargeter.retarget(frame)` called once per
 *                      captured frame): a latency path next to the throughput path of gmr_ik_solve
 *   gmr_evaluate       error1() / error2() (motion_retarget.py:188-200) and configuration.data.xpos / xquat
 *                      (mink.Configuration.update = mj_kinematics) at given qpos, without solving
 *   gmr_fk             KinematicsModel.forward_kinematics (kinematics_model.py:213-246)
 *   gmr_fk_shape       the same with `fitted_shape` (per-body scale of the local translations, kinematics_model.py:225)
 *   gmr_fk_min_height  the clip-global `torch.min(body_pos[..., 2])` of the height adjust
 *                      (scripts/smplx_to_robot_dataset.py:118-126)
 *   gmr_motion_epilogue, gmr_group_motion_epilogue  the whole post-processing after the retarget loop
 *                      (scripts/smplx_to_robot_dataset.py:93-131): root_rot / dof_pos out of qpos, local_body_pos, the height
 *                      adjust and the root-origin offset -- for one model, or for every member of a group in shared launches
 *   gmr_motion_track, gmr_group_motion_track  (no counterpart in the reference) what a consumer of the motion files does before it
 *                      trains a tracking policy: resampling to the controller's rate, world body poses, velocities
 *   gmr_motion_sample  (the reference's KinematicsModel in a trainer's loop: interpolation plus a torch loop over bodies per query)
 *                      the reference state of (clip, time) queries against a library of retargeted clips kept as qpos
 *   gmr_motion_contacts  (no counterpart in the reference) the per-frame foot-contact labels a tracking / AMP pipeline computes
 *                      from the export in a host loop, and the foot-slide and ground-penetration figures of a retargeted clip
 *   gmr_motion_footlock  (no counterpart in the reference) the foot-slide clean-up such a pipeline runs on the host: a loop over
 *                      contact phases with a small leg IK per frame, here a post-pass from qpos to qpos
 *   gmr_motion_dynamics  (no counterpart in the reference) what the consumers of the clips run on the host to filter them, MuJoCo's
 *                      inverse dynamics per frame: joint torques, the contact wrench on the root, centre of mass and ZMP, and per
 *                      clip torque-limit and ground-reaction statistics
 *   gmr_motion_self_collision  (no counterpart in the reference) the self-penetration filter the consumers of the clips run on the
 *                      host in a Python loop: FK plus a segment-segment distance per capsule pair and frame, and per clip the
 *                      deepest penetration, where it happens and for how long
 *   gmr_motion_self_collision_repair  (no counterpart in the reference) what such a consumer does with the colliding frames it
 *                      does not drop: a host loop that pushes the colliding capsule pairs apart over the hinges between them
 *   gmr_motion_mirror  (no counterpart in the reference) the left-right mirrored copy of every clip, the augmentation a tracking or
 *                      AMP pipeline doubles its data with: a signed permutation of the hinge columns and the reflected root
 *   gmr_motion_compose (no counterpart in the reference) long reference motions from segments of the clips: each segment moved
 *                      onto the end of the one before it in the plane and cross-faded into it
 *   gmr_motion_transitions (no counterpart in the reference) where such a segment may follow another: the motion-graph distance of
 *                      every window of the source clips to every window of the target clips, reduced to the best frame per pair
 *   gmr_motion_retime_plan, gmr_motion_retime_apply  (no counterpart in the reference) clips played slower exactly where a hinge
 *                      turns faster than its actuator can: a monotone time warp from per-joint velocity limits, and the clips
 *                      resampled along it at their own rate
 *   gmr_motion_retime_plan_torque  (no counterpart in the reference) the same warp from joint torques: a clip played slower
 *                      exactly where a hinge needs more torque than its actuator has
 *   gmr_dof_to_rot    KinematicsModel.dof_to_rot (kinematics_model.py:172-182; Joint.dof_to_rot :21-36)
 *   gmr_rot_to_dof     KinematicsModel.rot_to_dof (kinematics_model.py:184-197; Joint.rot_to_dof :38-53), clamped to the joint limits
 *   gmr_local_rot_to_global  KinematicsModel.convert_local_rot_to_global (kinematics_model.py:199-211)
 *   gmr_smplx_keypoints, gmr_smplx_keypoints_cols, gmr_smplx_keypoints_in  the numeric part of get_smplx_data_offline_fast (general_motion_retargeting/utils/smpl.py:109-198)
 *                      after the SMPL-X body model: slerp/lerp to the target frame rate, orientation chaining
 *   gmr_smplx_body     the SMPL-X body model's first 55 joints as load_smplx_file obtains them (general_motion_retargeting/utils/smpl.py:12-41):
 *                      rest joints from betas, the rigid chain over root_orient / pose_body, + trans -- all clips of a batch at once
 *   gmr_bvh_parse_header the HIERARCHY section of read_bvh (general_motion_retargeting/utils/lafan_vendor/extract.py:60-139)
 *   gmr_bvh_parse_motion, gmr_bvh_parse_motion_device  the MOTION block of read_bvh (general_motion_retargeting/utils/lafan_vendor/extract.py:140-166): the
 *                      per-line regex + float() loop that dominates BVH loading in the reference
 *   gmr_bvh_fk, gmr_bvh_fk_rows  the numeric part of load_lafan1_file (general_motion_retargeting/utils/lafan1.py:8-40):
 *                      euler_to_quat + quat_fk (utils/lafan_vendor/utils.py:56-103), Y-up -> Z-up, cm -> m,
 *                      LeftFootMod / RightFootMod synthesis
 */
#ifndef GMR_AMD_H
#define GMR_AMD_H

#include <stddef.h>
#include <stdint.h>

#include "gmr_blob.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GMR_ABI_VERSION 5

#define GMR_OK 0
#define GMR_EINVAL (-1)    /* bad argument / blob / shape                     */
#define GMR_EDEVICE (-2)   /* HIP runtime error (no device, launch failure)   */
#define GMR_EUNSUPPORTED (-3) /* model outside the kernel's limits            */
#define GMR_ENOCONFIG (-4) /* IK requested on a model compiled without tasks  */

#define GMR_DTYPE_F32 0
#define GMR_DTYPE_F64 1

typedef struct gmr_model gmr_model;

typedef struct gmr_model_info {
  int32_t nbody, nq, nv, nslot;
  int32_t ntask[2];
  int32_t n_active_dof; /* dofs with at least one task below them (the QP size)   */
  int32_t nv_padded;    /* compile-time system size of the kernel variant chosen  */
  int32_t lds_bytes;    /* dynamic LDS per sequence (one wavefront)               */
  int32_t device;
  int32_t reserved[6];
} gmr_model_info;

/* Per-call statistics written by gmr_ik_solve when stats != NULL (host memory). */
typedef struct gmr_ik_stats {
  int64_t n_items;        /* work items launched (one wavefront each)             */
  int64_t n_frames_total; /* frames processed, burn-in included                   */
  int64_t n_frames_out;   /* frames written                                       */
  int32_t reserved[4];
} gmr_ik_stats;

int gmr_abi_version(void);

/* blob: host pointer to a buffer in the layout of gmr_blob.h.  device: HIP device ordinal.
 * On failure returns NULL and, if err != NULL, writes a NUL-terminated message. */
gmr_model *gmr_model_create(const void *blob, size_t blob_bytes, int device, char *err, size_t err_len);
void gmr_model_destroy(gmr_model *m);
const char *gmr_last_error(const gmr_model *m);
int gmr_model_info_get(const gmr_model *m, gmr_model_info *out);

/* Per-joint velocity limit (mink.VelocityLimit as a box on the step of one QP solve): |dq_i| <= cap[i] in EVERY solve of every
 * launch of this model, intersected with the ConfigurationLimit box (no limit_gain on the cap).  cap = timestep * vmax.
 *   cap: host array of nv doubles in dof order, each > 0 or +inf; NULL switches the limit off (the state after create).
 *        GMR_EINVAL: an entry that is NaN, zero or negative, or a finite entry on one of the root's six dofs.
 * Takes effect for launches enqueued after it returns; must not be called while launches of this model are in flight.
 * gmr_ik_solve, gmr_ik_plan_order, gmr_ik_solve_ordered and the three group solves (each member's own cap) pick it up per call; a
 * session copies it at gmr_session_create and keeps that copy.  A capped launch runs the generic kernel instance.
 * gmr_model_get_step_cap returns GMR_OK and fills cap_out[nv] (+inf everywhere when the limit is off). */
int gmr_model_set_step_cap(gmr_model *m, const double *cap);
int gmr_model_get_step_cap(const gmr_model *m, double *cap_out);

/* Batched two-stage IK over work items.
 *   human_pos  device, [n_frames][n_cols][3] in_dtype, metres
 *   human_quat device, [n_frames][n_cols][4] in_dtype, wxyz
 *   slot_col   host,   [nslot] column (0..n_cols-1) of each slot of the model
 *   items      host,   [n_items] runs of consecutive frames (gmr_work_item)
 *   qpos_init  device, [*][nq] f64 or NULL (rows referenced by items[].init_row)
 *   qpos_final device, [*][nq] f64 or NULL (rows referenced by items[].final_row)
 *   qpos_out   device, [n_frames][nq] f64; only frames covered by an item's n_out are written
 *   iters_out  device, [n_frames] int32 or NULL: solve_ik calls spent on the frame
 *              (bit 30 set if a QP hit its iteration cap -- never expected; bit 31 if the frame's qpos has a
 *              non-finite coordinate, e.g. from non-finite key-points: callers can check a batch without reading qpos)
 *   frames_done device, [n_items] int32 or NULL: output frames each item solved (n_out unless a
 *              check_stride item stopped early, see gmr_blob.h)
 *   stream     hipStream_t (as void*), NULL = default stream.  The call is
 *              asynchronous with respect to the host ("Stream order", above).     */
int gmr_ik_solve(gmr_model *m, const void *human_pos, const void *human_quat, int in_dtype, int n_cols,
                 const int32_t *slot_col, int64_t n_frames, const gmr_work_item *items, int n_items,
                 const gmr_ik_params *params, const double *qpos_init, double *qpos_final, double *qpos_out,
                 int32_t *iters_out, int32_t *frames_done, gmr_ik_stats *stats, void *stream);

/* How gmr_ik_solve launches a batch: whole clips, one wavefront each from start to end, or -- plain clips of (nearly) equal
 * length, more of them than the device has wavefront slots -- cut into slices that wavefronts draw round-robin by ticket: a fixed
 * number of frames each through the clip, and ever shorter ones, halving down to a floor, over the last slice length of frames of
 * the longest clip, so that the launch's last round is short (csrc/slice_plan.h), the full solver state handed from slice to slice exactly, so that all clips advance at the same pace and
 * finish in the same last round whatever each costs.  Results are bit-identical either way.
 * gmr_ik_balance_plan is that choice as a pure host function (no device, no stream): the slice length in frames, or 0 for whole
 * clips.  Nonzero when every item is plain (no check_stride, no burn-in, no GMR_INIT_ROOT_TARGET start), n_items > slots (wavefront
 * slots of the device: 8 per compute unit), the standard deviation of the item lengths is at most 10 % of their mean, and the mean
 * is at least four slices.  Environment: GMR_AMD_BALANCE=0 never slices, GMR_AMD_BALANCE=1 slices every plain batch,
 * GMR_AMD_BALANCE=2 applies the rule above (the default, where DESIGN.md 8 says so), GMR_AMD_BALANCE_SLICE=<frames> overrides the
 * slice length, GMR_AMD_BALANCE_TAPER=<frames> the floor of the halving slices (0: fixed-length slices to the end; the function's
 * return value does not depend on it).  gmr_ik_solve_ordered and the group calls always run whole clips.
 * gmr_ik_sliced_timeouts: a waiting slice polls a bounded number of times; the bound only guards against a broken protocol.  A
 * wavefront that reaches it writes no frame and ends, as do the later slices of its clip (their rows of qpos_out and
 * frames_done stay as the caller left them), and this function -- host only, call it after synchronising the stream -- returns 1 if
 * that happened on the handle since its last call (it clears the word), else 0.  The cap grows with the slice length and with
 * the number of slices of one clip that can be resident at once, so a correct run stays orders of magnitude below it. */
int gmr_ik_balance_plan(const gmr_work_item *items, int n_items, int slots);
int gmr_ik_sliced_timeouts(gmr_model *m);

/* Launch order by predicted cost.  Work items start in array order (gmr_ik_solve puts longer items first); items of EQUAL
 * length still differ in cost -- solves per frame -- and with a few items per wavefront slot the start order decides how long the
 * last ones run alone (8192 clips x 3000 frames: 608 ms in array order, 549 ms most-expensive-first).
 *   gmr_ik_plan_order     solves the first probe_frames frames of every item for their cost only (nothing but order_out is
 *                         written) and orders the items by probe solves per frame x frames, most expensive first.
 *                         order_out device int32 [n_items]; other arguments as gmr_ik_solve; plain items only (no check_stride)
 *   gmr_ik_solve_ordered  gmr_ik_solve with workgroup b running item launch_order[b] (device int32 [n_items]; must be a
 *                         permutation of 0 .. n_items-1 -- entries outside that range are skipped, a repeated entry leaves another
 *                         item unsolved)
 * Both are asynchronous on `stream`; results are those of gmr_ik_solve bit for bit (the order only moves work in time).        */
int gmr_ik_plan_order(gmr_model *m, const void *human_pos, const void *human_quat, int in_dtype, int n_cols, const int32_t *slot_col,
                      int64_t n_frames, const gmr_work_item *items, int n_items, const gmr_ik_params *params, const double *qpos_init,
                      int probe_frames, int32_t *order_out, void *stream);
int gmr_ik_solve_ordered(gmr_model *m, const void *human_pos, const void *human_quat, int in_dtype, int n_cols, const int32_t *slot_col,
                         int64_t n_frames, const gmr_work_item *items, int n_items, const gmr_ik_params *params, const double *qpos_init,
                         double *qpos_final, double *qpos_out, int32_t *iters_out, int32_t *frames_done, gmr_ik_stats *stats,
                         const int32_t *launch_order, void *stream);

/* Several models in ONE launch (BASELINE config 4, "heterogeneous trees in one launch"): a group owns n models built for one
 * common kernel variant; gmr_group_ik_solve runs every member's work items in a single grid -- each wavefront looks up its
 * member's model, LDS layout and input / output arrays.  The reference analogue is one GeneralMotionRetargeting per robot in
 * the workers of one mp.Pool (scripts/smplx_to_robot_dataset.py:79-83, 241-242).
 *   gmr_group_create   blobs / blob_bytes host [n_models]: one packed model each (gmr_blob.h); NULL + message on failure
 *   gmr_group_model    borrowed handle of member i for everything else (gmr_fk, gmr_evaluate, sessions, gmr_ik_solve alone);
 *                      members are destroyed with the group
 *   gmr_group_ik_solve inputs host [n_models], member i's arguments exactly as gmr_ik_solve takes them (n_items = 0: no work
 *                      for that member); params are shared; asynchronous on `stream`
 * Cost-ordered group launch: gmr_ik_plan_order / gmr_ik_solve_ordered over all members' items together.  Both number the items
 * globally: item k of member i is base_i + k, base_i = the sum of n_items over the members before i (members without work add
 * nothing); order_out / launch_order are device int32 [sum of n_items].
 *   gmr_group_plan_order       probes the first probe_frames frames of every member's items in one grid and orders all of them
 *                              by probe solves per frame x frames, most expensive first, across robots; plain items only
 *                              (check_stride != 0: GMR_EINVAL)
 *   gmr_group_ik_solve_ordered gmr_group_ik_solve with workgroup b running global item launch_order[b] (a permutation of
 *                              0 .. total-1: entries outside that range are skipped, a repeated entry leaves another item
 *                              unsolved); results are those of gmr_group_ik_solve bit for bit                                  */
typedef struct gmr_group gmr_group;
typedef struct gmr_group_input {
  const void *human_pos, *human_quat; /* device */
  int32_t in_dtype, n_cols;
  const int32_t *slot_col;            /* host [nslot of member i] */
  int64_t n_frames;
  const gmr_work_item *items;         /* host [n_items] */
  int32_t n_items, reserved;
  const double *qpos_init;            /* device or NULL */
  double *qpos_final, *qpos_out;      /* device (qpos_final may be NULL) */
  int32_t *iters_out, *frames_done;   /* device or NULL */
} gmr_group_input;
gmr_group *gmr_group_create(const void *const *blobs, const size_t *blob_bytes, int n_models, int device, char *err, size_t err_len);
void gmr_group_destroy(gmr_group *g);
int gmr_group_size(const gmr_group *g);
gmr_model *gmr_group_model(gmr_group *g, int i);
const char *gmr_group_last_error(const gmr_group *g);
int gmr_group_ik_solve(gmr_group *g, const gmr_group_input *inputs, const gmr_ik_params *params, void *stream);
int gmr_group_plan_order(gmr_group *g, const gmr_group_input *inputs, const gmr_ik_params *params, int probe_frames, int32_t *order_out,
                         void *stream);
int gmr_group_ik_solve_ordered(gmr_group *g, const gmr_group_input *inputs, const gmr_ik_params *params, const int32_t *launch_order,
                               void *stream);

/* The dataset epilogue (what follows the solve in scripts/smplx_to_robot_dataset.py:93-131): per frame of a free-joint qpos
 * (layout [x y z qw qx qy qz hinges]), the arrays of the motion-file schema, bit for bit what the separate calls give:
 *   root_rot_out        qpos[:, [4,5,6,3]] (xyzw)                 dof_pos_out   qpos[:, 7:]
 *   local_body_pos_out  gmr_fk with root position 0 and the identity root rotation, dof = (float)qpos[:, 7:]
 *   root_pos_out        qpos[:, :3]; GMR_MOTION_HEIGHT_ADJUST: z = (z - (double)low_s) + ground_offset, low_s = the value
 *                       gmr_fk_min_height gives clip s for ((float)qpos[:, :3], (float)root_rot, (float)dof);
 *                       GMR_MOTION_ROOT_ORIGIN: xy minus the xy of the clip's first frame
 *   min_z_out           low_s per clip (+inf for an empty clip), or NULL
 * low_s is the minimum of the clip's body heights when all of them are ordered.  It is NaN when any of them is NaN (torch.min's
 * rule, and the reference script's).  +-inf take part in the minimum as values.
 * Non-finite input: a non-finite coordinate of qpos makes non-finite exactly the outputs that are arithmetic functions of it, and
 * changes no other output -- its own element of root_rot / dof_pos / root_pos, the bodies of its frame's local_body_pos below a
 * poisoned hinge, with GMR_MOTION_ROOT_ORIGIN the xy of its clip when it is the xy of the clip's first frame, and through low_s
 * (min_z_out[s], and with GMR_MOTION_HEIGHT_ADJUST the z of every frame of the clip) what the rule above says.
 * seq_offsets (host) start at 0, end at n_frames and never decrease (empty clips are allowed).  A planar-base model is refused
 * with GMR_EUNSUPPORTED, a model whose tile does not fit in LDS too.  Asynchronous on `stream`; the handle's device is selected.
 *   gmr_motion_epilogue        one model
 *   gmr_group_motion_epilogue  inputs host [group size]: member i's arguments (n_frames = 0: no work), all members in one grid  */
#define GMR_MOTION_HEIGHT_ADJUST 1
#define GMR_MOTION_ROOT_ORIGIN 2
typedef struct gmr_motion_input {
  const double *qpos;          /* device [n_frames][nq] f64, free-joint layout                    */
  int64_t n_frames;
  const int64_t *seq_offsets;  /* host [n_seq+1], 0 .. n_frames, non-decreasing (empty clips ok)  */
  int32_t n_seq, flags;        /* GMR_MOTION_* */
  double ground_offset;
  double *root_pos_out, *root_rot_out, *dof_pos_out;   /* device [n][3], [n][4] xyzw, [n][nq-7] f64 */
  float *local_body_pos_out;   /* device [n][nbody][3] f32 */
  float *min_z_out;            /* device [n_seq] f32 or NULL: low_s as gmr_fk_min_height gives it */
} gmr_motion_input;
int gmr_motion_epilogue(gmr_model *m, const gmr_motion_input *in, void *stream);
int gmr_group_motion_epilogue(gmr_group *g, const gmr_motion_input *inputs, void *stream);

/* The tracking export: solved free-joint qpos (layout [x y z qw qx qy qz hinges], concatenated clips) resampled to one output
 * rate, with every body's world pose and the velocities a tracking policy is trained on.  All arithmetic below is done as
 * written, without floating-point contraction.
 *
 * Resampling plan (host).  Clip s has T = seq_offsets[s+1] - seq_offsets[s] source frames at fps_in[s] and ratio[s] =
 * fps_in[s] / fps_out (a double).  It yields M_s = 0 output frames when T = 0, else M_s = floor((T-1) / ratio[s] + 1e-6) + 1;
 * out_offsets is the prefix sum of M_s.  The plan the caller passes is authoritative (any M_s >= 0, M_s = 0 where T = 0); the
 * kernel only clamps.  Output frame k of the clip reads the source frames
 *   u = (double)k * ratio[s],  i0 = min((int64)floor(u), T-1),  i1 = min(i0+1, T-1),  a = u - i0 when i1 > i0, else 0.
 * Resampled outputs, float64 [M][...], M = out_offsets[n_seq]:
 *   root_pos_out [M][3], joint_pos_out [M][nq-7]   x0 + a (x1 - x0)
 *   root_rot_out [M][4] xyzw                       shortest-arc slerp of q0, q1 (as xyzw): d = q0 . q1; d < 0: q1 = -q1, d = -d;
 *                                                  om = acos(min(d, 1)); (w0, w1) = (1-a, a) when om < 1e-8, else
 *                                                  (sin((1-a) om), sin(a om)) / sin(om); r = w0 q0 + w1 q1; r / |r|
 *   a = 0: all three are copies of frame i0, so at fps_out = fps_in they are qpos[:, :3], qpos[:, [4,5,6,3]] and qpos[:, 7:].
 *   q0 == q1 (all four components): root_rot_out is a copy of q0 for every a -- a standing robot's rows are all the same row.
 * World body states, float32: body_pos_w_out [M][nbody][3], body_quat_w_out [M][nbody][4] xyzw: bit for bit what gmr_fk
 * returns for the float32 casts of root_pos_out, root_rot_out and joint_pos_out.
 * Velocities, dt = 1 / fps_out, within a clip km = max(k-1, 0), kp = min(k+1, M_s-1), h = (kp - km) dt; every velocity is 0
 * when h = 0 (a clip of one output frame); no difference crosses a clip:
 *   root_lin_vel_out [M][3], joint_vel_out [M][nq-7] f64   (x[kp] - x[km]) / h
 *   root_ang_vel_out [M][3] f64, world frame               rotvec(q[kp] (x) conj(q[km])) / h, where for p (x) conj(q) = (v, w):
 *                                                          w = pw qw + (pv . qv), v = qw pv - pw qv - pv x qv; negate both
 *                                                          when w < 0; n = |v|; rotvec = v (2 atan2(n, w) / n) when
 *                                                          n > 1e-12, else 2 v
 *   body_lin_vel_w_out, body_ang_vel_w_out [M][nbody][3] f32   the same two formulas on the float32 body_pos_w / body_quat_w,
 *                                                          promoted to double, the result rounded to float32 once
 * Non-finite input: a non-finite coordinate of qpos makes non-finite exactly the outputs that are arithmetic functions of it, and
 * changes no other output: the output frames k that read its source frame as i0, or as i1 with a > 0 (a = 0 is a copy of frame
 * i0), and, in the velocity arrays, their neighbours k-1 and k+1 inside the clip.  The formulas decide which elements: r / |r| of
 * an r with one infinite component is 0 in the other three, and every comparison with a NaN is false (min(d, 1) of a NaN d is 1).
 * Any output may be NULL; without any of the four body outputs the FK is skipped.  seq_offsets follow gmr_motion_input's
 * rules.  GMR_EINVAL: fps_out <= 0, a ratio <= 0 (fps_in <= 0), out_offsets that do not start at 0, decrease, or give output
 * frames to a clip without source frames.  A planar-base model is refused with GMR_EUNSUPPORTED, a model whose tile does not
 * fit in LDS too.  Asynchronous on `stream`; the handle's device is selected.
 *   gmr_motion_track        one model
 *   gmr_group_motion_track  inputs host [group size]: member i's arguments (n_frames = 0: no work), all members in one grid
 *
 * The low-pass (lowpass_hz > 0): qpos is first filtered per clip with a zero-phase 2nd-order Butterworth low-pass, forward and
 * backward (scipy.signal.filtfilt of scipy.signal.butter(2, 2 fc / fs)), on the device.  lowpass_hz = 0 (also -0) leaves the
 * call exactly as described above.  All arithmetic is done as written, in float64, without contraction.
 * Coefficients.  For clip s, fs = ratio[s] * fps_out (this product, in double) and fc = (double)lowpass_hz;
 *   K = tan(pi fc / fs), n = 1 / (1 + sqrt(2) K + K K),
 *   b0 = K K n, b1 = 2 b0, b2 = b0, a1 = 2 (K K - 1) n, a2 = (1 - sqrt(2) K + K K) n
 * as gmr_lowpass_coefficients below returns them (the call uses that function for every clip).  Applied forward and backward
 * the filter is -6 dB at fc, exactly as filtfilt is; no cutoff correction is applied.
 * One column x[0..T-1] of one clip.  T <= 1: a copy.  Otherwise e = min(9, T - 1) (scipy's padlen = 3 * 3, shortened for the
 * clips scipy would refuse), and the odd extension is
 *   ext = [2 x[0] - x[e], ..., 2 x[0] - x[1], x[0..T-1], 2 x[T-1] - x[T-2], ..., 2 x[T-1] - x[T-1-e]].
 * One pass is the transposed direct form II, y = b0 x + z1; z1 = (b1 x - a1 y) + z2; z2 = b2 x - a2 y, started at
 * z1 = (1 - b0) u, z2 = (b2 - a2) u with u the first sample of the pass (lfilter_zi times the first sample).  The forward pass
 * runs over ext, the backward pass over the forward result reversed; the output is the middle T samples.
 * Columns.  x y z and every hinge are filtered as above.  The root quaternion (columns 3..6, wxyz) is first made
 * sign-continuous along the clip: q'_0 = q_0, and q'_i = -q_i when q'_{i-1} . q_i < 0, else q_i, the dot product being
 * ((w w + x x) + y y) + z z.  The four components of q' are filtered like any other column (T = 1: copied), and the result r
 * leaves as r / sqrt(((rw rw + rx rx) + ry ry) + rz rz).  The filtered quaternion is therefore sign-continuous, and negating
 * any input rows other than row 0 changes no output bit.  There is no clamp to the joint ranges.
 * The export.  All ten outputs are, bit for bit, what the same call with lowpass_hz = 0 gives on the filtered qpos.
 * Non-finite input.  A non-finite coordinate makes non-finite every frame of its own column of its own clip (the backward
 * pass starts from what the forward pass ended with); in the root quaternion it makes non-finite all four columns of that clip
 * (a NaN norm).  It changes no other column and no other clip.  The export's own rule applies from there.
 * Errors.  GMR_EINVAL for a negative or non-finite lowpass_hz and for any clip with source frames and lowpass_hz >= fs / 2
 * (the message names the clip, and in a group the member); GMR_EUNSUPPORTED when nq > 64 (no registry robot exceeds 50).
 * Memory.  With the filter on the call takes n_frames * nq * 8 bytes of stream-ordered scratch per filtered member on the
 * call's stream (the filtered qpos), released behind the launches, and enqueues one more kernel.  */

/* The five coefficients gmr_motion_track uses for a clip sampled at fs with cutoff cutoff_hz: c = {b0, b1, b2, a1, a2}.
 * GMR_EINVAL unless 0 < cutoff_hz < fs / 2 and both are finite.  Host only: no stream, no device work. */
int gmr_lowpass_coefficients(double cutoff_hz, double fs, double *c);

typedef struct gmr_track_input {
  const double *qpos;          /* device [n_frames][nq] f64, free-joint layout                    */
  int64_t n_frames;
  const int64_t *seq_offsets;  /* host [n_seq+1], 0 .. n_frames, non-decreasing (empty clips ok)  */
  const int64_t *out_offsets;  /* host [n_seq+1], the plan: 0 .. M, non-decreasing                */
  const double *ratio;         /* host [n_seq], fps_in[s] / fps_out                               */
  double fps_out;
  int32_t n_seq;
  float lowpass_hz;            /* cutoff of the zero-phase low-pass applied to qpos first; 0 (all-zero bits, or -0): off */
  double *root_pos_out, *root_rot_out, *joint_pos_out;          /* device [M][3], [M][4] xyzw, [M][nq-7] f64 */
  double *root_lin_vel_out, *root_ang_vel_out, *joint_vel_out;  /* device [M][3], [M][3], [M][nq-7] f64      */
  float *body_pos_w_out, *body_quat_w_out;                      /* device [M][nbody][3], [M][nbody][4] xyzw f32 */
  float *body_lin_vel_w_out, *body_ang_vel_w_out;               /* device [M][nbody][3] f32 */
} gmr_track_input;
int gmr_motion_track(gmr_model *m, const gmr_track_input *in, void *stream);
int gmr_group_motion_track(gmr_group *g, const gmr_track_input *inputs, void *stream);

/* The motion library's random access: Q queries (clip, time) against solved free-joint qpos (layout [x y z qw qx qy qz hinges],
 * concatenated clips), each answered with the interpolated generalized state, its velocity, and the world poses and twists of
 * the bodies that are asked for.  All arithmetic below is done as written, without floating-point contraction.  "The export"
 * is gmr_motion_track above; lerp(x0, x1, a) is its x0 + a (x1 - x0) with a = 0 a copy of x0, slerp its shortest-arc slerp,
 * angvel(p, q, h) its rotvec(p (x) conj(q)) / h.
 *
 * Query j: clip s = ids[j / k_per_id], time t = times[j] in seconds from the clip's first frame (a float32 t is promoted to
 * double first).  T = seq_offsets[s+1] - seq_offsets[s], f = fps[s].
 *   u = t f;  i0 = 0 when u <= 0, T-1 when u >= T-1, else floor(u);  i1 = min(i0+1, T-1);
 *   a = u - i0 when i1 > i0 and 0 < u, else 0.
 * Pose, the export's formula on the rows i0, i1 and the weight a, under the same conditions:
 *   root_pos_out [Q][3], joint_pos_out [Q][nq-7]   lerp(x[i0], x[i1], a)
 *   root_rot_out [Q][4] xyzw                       slerp(q[i0], q[i1], a); a copy of q[i0] when a = 0 or when q[i0] == q[i1]
 * Generalized velocity, continuous in t, and at an integer frame the export's value at equal rates.  For a source frame i:
 * km = max(i-1, 0), kp = min(i+1, T-1), h = (double)(kp - km) * (1.0 / f), and
 *   v_i = (x[kp] - x[km]) / h,  w_i = angvel(q[kp], q[km], h) (q as xyzw),  both 0 when h = 0;
 *   root_lin_vel_out [Q][3], joint_vel_out [Q][nq-7]   lerp(v_i0, v_i1, a)
 *   root_ang_vel_out [Q][3], world frame               lerp(w_i0, w_i1, a), componentwise
 * A query reads at most the four rows i0-1, i0, i1, i1+1, clamped to its clip; nothing crosses a clip.
 * The six generalized outputs have the element type out_dtype: the float64 value, or its single rounding to float32.
 * World body states, float32 whatever out_dtype is; column c of a query is body body_ids[c] (body_ids NULL: all bodies in model
 * order, n_sel = 0, and nbody columns):
 *   body_pos_w_out [Q][n_sel][3], body_quat_w_out [Q][n_sel][4] xyzw   bit for bit what gmr_fk returns for the float32 casts of
 *                                                  the float64 root_pos, root_rot and joint_pos of the query
 *   body_lin_vel_w_out, body_ang_vel_w_out [Q][n_sel][3]   the twist the generalized velocity gives the body at that pose,
 *       carried down gmr_fk's chain in float32 from the root's v = (float)root_lin_vel, w = (float)root_ang_vel (float64 values).
 *       For body j with parent p, x and R the chain's own position and rotation (xyzw quaternion r), thetadot = (float)joint_vel:
 *         d = x_j - x_p (componentwise);  v_j = v_p + (w_p x d),  (w x d)_x = w_y d_z - w_z d_y and cyclic;
 *         w_j = w_p + (R_j axis_j) thetadot_j componentwise, w_j = w_p for a body without a hinge;  axis_j = (float) of the unit
 *         axis, R axis = gmr_fk's quat_rotate(r, axis): axis (2 r_w^2 - 1) + (r_v x axis) r_w 2 + r_v (r_v . axis) 2.
 * Invalid query: id < 0, id >= n_seq, T = 0, a non-finite time (or a NaN u, from a NaN fps).  Every output element of the query
 * is NaN and no row of qpos is read for it: the only bounds protection for ids that arrive on the device, for any int64 value.
 * Non-finite qpos rows: rows the query reads make non-finite exactly the outputs that are arithmetic functions of them (the
 * export's rule: a = 0 is a copy of row i0 and of v_i0, w_i0); no other query is affected.
 * GMR_EINVAL: k_per_id < 1, n_queries not a multiple of k_per_id, a negative count, n_sel < 0, body_ids NULL with n_sel != 0, an
 * unknown dtype.  GMR_EUNSUPPORTED: a planar-base model, or one whose per-wavefront LDS exceeds 160 KB.  n_queries = 0 returns
 * GMR_OK without a launch.  Any output may be NULL; without any of the four body outputs the chain is skipped.  body_ids is
 * trusted (each 0 <= id < nbody): range checking is the caller's job.
 * A call enqueues one kernel and nothing else: no allocation, no host-to-device copy, no synchronisation -- the clip table
 * (seq_offsets, fps), ids and times are device arrays and this struct travels as the kernel's argument.  Asynchronous on
 * `stream`; the handle's device is selected.
 * Layout (LP64): sizeof 168; offsets qpos 0, n_frames 8, seq_offsets 16, fps 24, n_seq 32, k_per_id 36, ids 40, times 48,
 * time_dtype 56, out_dtype 60, n_queries 64, body_ids 72, n_sel 80, reserved 84, root_pos_out 88, root_rot_out 96,
 * joint_pos_out 104, root_lin_vel_out 112, root_ang_vel_out 120, joint_vel_out 128, body_pos_w_out 136, body_quat_w_out 144,
 * body_lin_vel_w_out 152, body_ang_vel_w_out 160.  */
typedef struct gmr_sample_input {
  const double  *qpos;         /* device [n_frames][nq] f64, free-joint layout, concatenated clips */
  int64_t        n_frames;
  const int64_t *seq_offsets;  /* DEVICE [n_seq+1] */
  const double  *fps;          /* DEVICE [n_seq], > 0 */
  int32_t        n_seq, k_per_id;       /* k_per_id >= 1: query j uses ids[j / k_per_id] */
  const int64_t *ids;          /* device [n_queries / k_per_id] */
  const void    *times;        /* device [n_queries], seconds from the clip's first frame */
  int32_t        time_dtype, out_dtype; /* GMR_DTYPE_F32 / F64: times; the six generalized outputs */
  int64_t        n_queries;
  const int32_t *body_ids;     /* device [n_sel] body indices, or NULL = all bodies in model order */
  int32_t        n_sel, reserved;
  void  *root_pos_out, *root_rot_out, *joint_pos_out;           /* [Q][3], [Q][4] xyzw, [Q][nq-7] */
  void  *root_lin_vel_out, *root_ang_vel_out, *joint_vel_out;   /* [Q][3], [Q][3], [Q][nq-7]      */
  float *body_pos_w_out, *body_quat_w_out;                      /* [Q][n_sel][3], [Q][n_sel][4] xyzw f32 */
  float *body_lin_vel_w_out, *body_ang_vel_w_out;               /* [Q][n_sel][3] f32 */
} gmr_sample_input;
int gmr_motion_sample(gmr_model *m, const gmr_sample_input *in, void *stream);

/* Foot-contact labels and slide statistics of a tracking export: which of C chosen bodies are on the ground in which frame --
 * near the ground, slow, with hysteresis -- and per clip how far a planted body slides and how deep it goes below the ground.
 * All arithmetic below is done as written, in float64, without floating-point contraction.
 *
 * Inputs, all device arrays; the call enqueues one kernel and nothing else: no allocation, no copy, no synchronisation.  The
 * whole call is this struct, its stream included (in->stream: the call's stream, in the sense of the stream-order paragraph at
 * the top of this file); the struct is read completely before the call returns.
 *   body_pos_w, body_lin_vel_w  float32 [n_rows][nbody][3]: what gmr_motion_track wrote, or any arrays of that shape (M = n_rows)
 *   out_offsets                 int64 [n_seq+1]: clip s owns the rows a = clamp(out_offsets[s], 0, M) to
 *                               b = clamp(out_offsets[s+1], a, M), M_s = b - a.  The kernel only clamps.
 *   body_ids                    int32 [C], C = n_contact, 1 <= C <= 64.  Trusted, as in gmr_motion_sample.
 *   height_offset               float64 [C], or NULL for all zeros: the height of the body origin above its own sole
 *   ground_mode, ground_z       GMR_CONTACT_GROUND_FIXED or GMR_CONTACT_GROUND_CLIP_MIN; the ground height of the fixed mode
 *   height_on, height_off, speed_on, speed_off   the thresholds, metres and metres per second
 * Per clip s, frame k = 0 .. M_s-1 (row g = a + k), contact column c (body j = body_ids[c]):
 *   hc = (double)body_pos_w[g][j][2] - height_offset[c]
 *   base_s = ground_z in the fixed mode.  In the CLIP_MIN mode the minimum of hc over all k and all c of the clip: NaN when
 *            any hc is NaN (torch.min's rule, the one gmr_fk_min_height follows); +-inf take part as values.
 *   h = hc - base_s;  s2 = (vx vx + vy vy) + vz vz of the promoted body_lin_vel_w[g][j]
 *   enter = h <= height_on && s2 <= speed_on * speed_on;  stay = h <= height_off && s2 <= speed_off * speed_off
 *   the label starts at c_{-1} = 0; then c_k = 1 when enter, 0 when !stay, and c_{k-1} otherwise.
 * Every comparison with a NaN is false: a non-finite frame is off, and a clip with a NaN base_s is off everywhere.
 * Outputs, any may be NULL; d_k = sqrt(dx dx + dy dy) with dx = (double)x_k - (double)x_{k-1} and dy likewise:
 *   contact_out [n_rows][C] u8           c_k, 0 or 1
 *   frames_out [n_seq][C] i32            sum of c_k over the clip
 *   touchdowns_out [n_seq][C] i32        number of k with c_k = 1 and c_{k-1} = 0
 *   slide_sum_out [n_seq][C] f64         sum of d_k over k >= 1 with c_k = c_{k-1} = 1
 *   slide_step_max_out [n_seq][C] f64    sqrt of the maximum of (dx dx + dy dy) over the same k; 0 when there is none
 *   depth_max_out [n_seq][C] f64         running r = 0; r = (base_s - hc_k) > r ? (base_s - hc_k) : r
 *   airborne_frames_out [n_seq] i32      number of k with c_k = 0 in every column
 *   base_out [n_seq] f64                 base_s; for M_s = 0 in the CLIP_MIN mode it is NaN
 * A clip without frames reports 0 everywhere else.  Nothing crosses a clip.  A non-finite element changes no output of another
 * clip; within its own clip in the fixed mode it changes only its own column, plus airborne_frames.  Rows outside every clip
 * are not written.  slide_sum is reduced in a fixed order (64-frame tiles, added tile by tile): a report is bit-reproducible.
 * GMR_EINVAL: a threshold that is not finite, height_on > height_off, speed_on < 0, speed_on > speed_off, C < 1, an unknown
 * mode, a non-finite ground_z in the fixed mode, NULL inputs with M > 0, negative counts.  GMR_EUNSUPPORTED: C > 64.  M = 0 or
 * n_seq = 0 returns GMR_OK without a launch.  Asynchronous on in->stream; the handle's device is selected.
 * Layout (LP64): sizeof 176; offsets body_pos_w 0, body_lin_vel_w 8, n_rows 16, out_offsets 24, body_ids 32, height_offset 40,
 * n_seq 48, n_contact 52, ground_mode 56, reserved 60, ground_z 64, height_on 72, height_off 80, speed_on 88, speed_off 96,
 * stream 104, contact_out 112, frames_out 120, touchdowns_out 128, slide_sum_out 136, slide_step_max_out 144,
 * depth_max_out 152, airborne_frames_out 160, base_out 168.  */
#define GMR_CONTACT_GROUND_FIXED 0
#define GMR_CONTACT_GROUND_CLIP_MIN 1
typedef struct gmr_contact_input {
  const float   *body_pos_w;      /* device [n_rows][nbody][3] f32 */
  const float   *body_lin_vel_w;  /* device [n_rows][nbody][3] f32 */
  int64_t        n_rows;
  const int64_t *out_offsets;     /* DEVICE [n_seq+1] */
  const int32_t *body_ids;        /* device [n_contact] body indices */
  const double  *height_offset;   /* device [n_contact], or NULL = zeros */
  int32_t        n_seq, n_contact;
  int32_t        ground_mode, reserved;
  double         ground_z;
  double         height_on, height_off, speed_on, speed_off;
  void          *stream;          /* the call's stream */
  uint8_t       *contact_out;
  int32_t       *frames_out, *touchdowns_out;
  double        *slide_sum_out, *slide_step_max_out, *depth_max_out;
  int32_t       *airborne_frames_out;
  double        *base_out;
} gmr_contact_input;
int gmr_motion_contacts(gmr_model *m, const gmr_contact_input *in);

/* Foot locking: remove the horizontal slide of planted feet from retargeted qpos.  Per contact column the body is pinned, over
 * every planted run, to the mean of its own xy; the shift is blended out over W frames on both sides of a run; a damped
 * least-squares iteration over the column's own hinges moves the body there.  Heights and orientations stay: this removes slide,
 * not penetration.  All arithmetic below is done as written, in float64, without floating-point contraction; a - b - c means
 * (a - b) - c.
 *
 * The whole call is this struct, its stream included (in->stream, in the sense of the stream-order paragraph at the top of this
 * file); the struct and body_ids are read completely before the call returns.  The call enqueues three kernels on in->stream and
 * nothing else: no allocation, no copy, no synchronisation.  pos_out and shift_out are also the kernels' exchange.
 *   qpos          device f64 [n_frames][nq], free-joint layout (x y z, qw qx qy qz, hinges), concatenated clips (N = n_frames)
 *   seq_offsets   DEVICE int64 [n_seq+1]: clip s owns the rows a = clamp(seq_offsets[s], 0, N) to b = clamp(seq_offsets[s+1], a, N).
 *                 The kernels only clamp; clips that overlap race with each other.
 *   contact       device u8 [n_frames][C]: non-zero = planted; labels at qpos's own frames
 *   body_ids      HOST int32 [C], C = n_contact, 1 <= C <= 8, read and validated before the call returns
 *   blend_frames  W >= 0;  min_run >= 1;  iterations I, 1 .. 32;  damping = lambda^2 > 0 (m^2);  step_cap > 0 (rad)
 * Chains.  The path of column c is the bodies from body_ids[c] up to, not including, the root, taken root side first; its chain is
 * the hinges on that path that lie on no other column's path (a shared waist joint is never moved, nor is the root).
 * FK of column c at the angles th (MuJoCo's convention, what gmr_evaluate reports as xpos): x = qpos[0..2], r = qpos[3..6] / n with
 * n = sqrt(qw qw + qx qx + qy qy + qz qz); then per path body j: x = x + rot(r, pos_j), r = r (x) quat_j, and for a hinge
 * r = r (x) [cos(th_j / 2), sin(th_j / 2) axis_j].  (a (x) b).w = a.w b.w - a.x b.x - a.y b.y - a.z b.z, .x = a.w b.x + a.x b.w +
 * a.y b.z - a.z b.y, .y = a.w b.y - a.x b.z + a.y b.w + a.z b.x, .z = a.w b.z + a.x b.y - a.y b.x + a.z b.w.  rot(q, v) = v + q.w t +
 * (q.xyz x t) with t = 2 (q.xyz x v), every cross product as (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x).
 * Per clip s, frame k = 0 .. M_s-1 (row g = a + k), column c:
 *   valid[k]  all nq entries of the row are finite
 *   L[k]      contact[g][c] != 0 && valid[k]
 *   p[k]      the FK above at the row's own angles
 *   runs      maximal intervals of L = 1 inside the clip; a run shorter than min_run counts as L = 0.  Nothing crosses a clip.
 *   anchor    A = (sx / n, sy / n) over the run's n frames.  sx: per 64-frame tile of the clip (frames 64 t .. 64 t + 63 counted
 *             from the clip's first) the run's p.x at their positions in the tile and zeros elsewhere, summed by the balanced binary
 *             tree (neighbours first); the tiles the run touches are added to 0.0 in ascending order.  sy likewise.
 *   inside a run   d[k] = (A.x - p.x, A.y - p.y, 0)
 *   outside, valid frames   e = the last frame of the nearest run before k, f = the first frame of the nearest run after k (same clip
 *             and column).  w- = S(1 - (k - e) / (W + 1)) when e exists and k - e <= W, else 0; w+ = S(1 - (f - k) / (W + 1)) when
 *             f exists and f - k <= W, else 0; S(t) = t t (3 - 2 t).  d[k] = (w- d[e] + w+ d[f]) / max(1, w- + w+), a side
 *             without weight adding 0.0; no shift when both are 0.
 *   solve     every valid frame inside a run or with a weight.  t = (p.x + d.x, p.y + d.y, p.z); q = the row's own chain angles q0;
 *             exactly I times, no early exit:  e = t - p(q);  J_i = w_i x (p(q) - o_i) for the chain's hinges, root side first, w_i
 *             = rot(r_i, axis_i) and o_i = x_i the hinge body's world pose;  G = J J^T (each entry summed over i in that order from
 *             0.0) + lambda^2 on the diagonal;  Cholesky l00 = sqrt(g00), l10 = g10 / l00, l20 = g20 / l00, l11 = sqrt(g11 - l10
 *             l10), l21 = (g21 - l20 l10) / l11, l22 = sqrt(g22 - l20 l20 - l21 l21);  z0 = e0 / l00, z1 = (e1 - l10 z0) / l11,
 *             z2 = (e2 - l20 z0 - l21 z1) / l22;  y2 = z2 / l22, y1 = (z1 - l21 y2) / l11, y0 = (z0 - l10 y1 - l20 y2) / l00;
 *             dq_i = J_i0 y0 + J_i1 y1 + J_i2 y2;  m = max |dq_i|, scale = m > step_cap ? step_cap / m : 1;
 *             q_i = clamp(q_i + scale dq_i, min(lo_i, q0_i), max(hi_i, q0_i)) for a limited hinge, unclamped otherwise.
 * Outputs, device arrays:
 *   qpos_out [n_frames][nq] f64          the rows with the solved chain angles.  Every other entry -- the root's seven, hinges outside
 *                                        the chains, frames that are not solved, invalid frames -- is copied bit for bit.  Must not
 *                                        alias qpos
 *   pos_out [n_frames][C][3] f64         p; NaN in an invalid frame.  Required
 *   shift_out [n_frames][C][3] f64       d, zero where there is none.  Required
 *   runs_out [n_seq][C] i32              runs of at least min_run frames; may be NULL
 *   locked_frames_out [n_seq][C] i32     frames inside them; may be NULL
 *   shift_max_out [n_seq][C] f64         sqrt of the maximum of d.x d.x + d.y d.y over the solved frames; may be NULL
 *   residual_max_out [n_seq][C] f64      maximum of sqrt(ex ex + ey ey + ez ez), e = t - p(q) after the last iteration; may be NULL
 *   limit_frames_out [n_seq][C] i32      solved frames in which a limited chain hinge ends on its widened bound; may be NULL
 * A clip without frames reports 0.  Rows outside every clip are not written.  A non-finite row changes no output byte of another
 * clip; within its own clip it is copied through and only splits runs.  Two calls give identical bytes.
 * GMR_EINVAL: a body id out of range or named twice, a chain of fewer than 3 hinges, C outside 1 .. 8, W < 0, min_run < 1, I outside
 * 1 .. 32, damping or step_cap not finite and > 0, qpos_out == qpos, NULL arrays with work to do, negative counts.
 * GMR_EUNSUPPORTED: a planar-base model, a chain of more than 16 hinges, a contact body more than 32 bodies below the root.  These
 * are checked before anything is enqueued.  n_frames = 0 or n_seq = 0 returns GMR_OK without a launch.  Asynchronous on
 * in->stream; the handle's device is selected.
 * Layout (LP64): sizeof 152; offsets qpos 0, n_frames 8, seq_offsets 16, contact 24, body_ids 32, n_seq 40, n_contact 44,
 * blend_frames 48, min_run 52, iterations 56, reserved 60, damping 64, step_cap 72, stream 80, qpos_out 88, pos_out 96,
 * shift_out 104, runs_out 112, locked_frames_out 120, shift_max_out 128, residual_max_out 136, limit_frames_out 144.  */
typedef struct gmr_footlock_input {
  const double  *qpos;            /* device [n_frames][nq] f64 */
  int64_t        n_frames;
  const int64_t *seq_offsets;     /* DEVICE [n_seq+1] */
  const uint8_t *contact;         /* device [n_frames][n_contact] u8 */
  const int32_t *body_ids;        /* HOST [n_contact] body indices */
  int32_t        n_seq, n_contact;
  int32_t        blend_frames, min_run;
  int32_t        iterations, reserved;
  double         damping, step_cap;
  void          *stream;          /* the call's stream */
  double        *qpos_out;
  double        *pos_out, *shift_out;
  int32_t       *runs_out, *locked_frames_out;
  double        *shift_max_out, *residual_max_out;
  int32_t       *limit_frames_out;
} gmr_footlock_input;
int gmr_motion_footlock(gmr_model *m, const gmr_footlock_input *in);

/* Inverse dynamics of retargeted qpos with a floating base: per frame the joint torques the motion needs, the wrench the contacts
 * must supply on the root, the centre of mass and the zero-moment point; per clip torque-limit and ground-reaction statistics.
 * All arithmetic is float64 without floating-point contraction; a + b + c means (a + b) + c.
 *
 * The whole call is this struct, its stream included (in->stream, in the sense of the stream-order paragraph at the top of this
 * file); the struct is read completely before the call returns.  The call enqueues two kernels on in->stream (one when no
 * statistic is asked for) and nothing else: no allocation, no copy, no synchronisation.  All arrays are device arrays.
 *   qpos          f64 [n_frames][nq], free-joint layout (x y z, qw qx qy qz, hinges), concatenated clips (N = n_frames)
 *   seq_offsets   int64 [n_seq+1]: clip s owns the rows a = clamp(seq_offsets[s], 0, N) to b = clamp(seq_offsets[s+1], a, N), T = b - a
 *   fps           one rate for the call, h = 1 / fps
 *   gravity_x/y/z the gravity vector g in m/s^2, usually (0, 0, -9.81);  ground_z: the height of the ground plane of the ZMP
 *   fz_min        a frame whose F_z is below fz_min (sum m) |g| is "unloaded".  0.05 is a convention, not measured on any robot
 *   qvel, qacc    f64 [n_frames][nv] or NULL, nv = nq - 1: entries 0..2 the root's linear part in the world frame, 3..5 the root's
 *                 angular part IN THE WORLD FRAME -- the convention gmr_motion_track writes, not MuJoCo's local-frame qvel[3..5] --
 *                 then the hinges.
 * The inertial table, in the model's body order (nbody must equal the model's): body_parent int32 [nbody] (-1 for the root; the
 * bodies are in depth-first order, so a subtree is a run of indices), body_mass [nbody], body_com [nbody][3] (centre of mass in the
 * body frame), body_inertia [nbody][6] (xx yy zz xy xz yz about the centre of mass, body frame), armature [nq-7] and torque_limit
 * [nq-7] in qpos order (> 0, +inf for none).  Trusted, as body_ids are in gmr_motion_sample; the kernel only clamps body_parent.
 * Velocity when qvel is NULL: the tracking export's central differences.  Frame k of a clip: km = max(k-1, 0), kp = min(k+1, T-1),
 * hv = (double)(kp - km) h; linear and hinge parts (x[kp] - x[km]) / hv, angular part rotvec(q[kp] (x) conj(q[km])) / hv with
 * gmr_motion_track's rotvec on the rows as they are (wxyz); all 0 when hv = 0.
 * Acceleration when qacc is NULL: 0 for T < 3; else with kc = clamp(k, 1, T-2) (the first and last frame take their neighbour's)
 * linear and hinge parts ((x[kc+1] - 2 x[kc]) + x[kc-1]) / (h h), angular part (w+ - w-) / h with
 * w+ = rotvec(q[kc+1] (x) conj(q[kc])) / h and w- = rotvec(q[kc] (x) conj(q[kc-1])) / h.
 * Poses are gmr_motion_footlock's FK (MuJoCo's convention, the root quaternion divided by its norm), not the float32 gmr_fk.  Body i
 * has mass m_i, world centre of mass c_i, world rotation R_i, body-frame inertia I_i and angular velocity w_i; the velocity (v, w)
 * and acceleration of the root above and the hinge rates carry down the tree as rigid-body kinematics.  For a point p let
 *   W(p, set) = sum over i in set of (c_i - p) x m_i (c_i'' - g) + d/dt(R_i I_i R_i^T w_i).
 * Outputs per frame, any may be NULL:
 *   tau_out [n_frames][nq-7]       a_j . W(p_j, subtree(j)) + armature_j theta_j'', a_j the hinge's world axis, p_j its world anchor
 *   root_wrench_out [n_frames][6]  (F, M): F = sum over all i of m_i (c_i'' - g), M = W(p_root, all).  Dual to the root's (v, w): the
 *                                  power of the motion is F . v + M . w + tau . theta'
 *   com_out [n_frames][3]          sum m_i c_i / sum m_i
 *   zmp_out [n_frames][2]          ((ground_z F_x - Mo_y) / F_z, (Mo_x + ground_z F_y) / F_z) with Mo = M + p_root x F; both NaN in
 *                                  an unloaded frame
 *   qvel_out, qacc_out [n_frames][nv]   the velocity and acceleration used, given or differenced
 * Every sum over bodies runs in body order from 0.0, moments are gathered about p_root; how the kernel walks the tree is its own
 * business and results agree with the formula to rounding.
 * Per-clip statistics, any may be NULL, reduced by the second kernel from tau_out and root_wrench_out (both are required when a
 * statistic is asked for).  A frame with a non-finite entry in its tau or root_wrench row is counted in nonfinite_frames and takes
 * part in no other statistic.  Over the other frames of the clip, hinges in qpos order:
 *   tau_abs_max_out, tau_rms_out [n_seq][nq-7] f64   max |tau|; sqrt(sum tau^2 / frames), the sum added frame by frame from 0.0
 *   tau_ratio_max_out [n_seq][nq-7] f64              max |tau| / torque_limit (0 for a hinge without a limit)
 *   frames_over_limit_out [n_seq][nq-7] i32          frames with |tau| > torque_limit
 *   frames_any_over_limit_out [n_seq] i32            frames in which any hinge is over its limit
 *   fz_ratio_max_out, fz_ratio_min_out [n_seq] f64   extremes of F_z / ((sum m) |g|), 0 without a finite frame
 *   unloaded_frames_out, nonfinite_frames_out [n_seq] i32
 * A clip without frames reports 0.  Rows outside every clip are not written.  Two calls give identical bytes.  Non-finite input: a
 * non-finite entry of a qpos row reaches only the frames whose stencil reads that row, and only its own clip's statistics; no byte
 * of another clip changes.
 * GMR_EINVAL: fps, gravity, ground_z or fz_min not finite, fps <= 0, fz_min < 0, a zero gravity, NULL arrays with work to do, a
 * statistic without tau_out and root_wrench_out, negative counts.  GMR_EUNSUPPORTED: a planar-base model, nbody that is not the
 * model's, a model of more than 64 bodies (its work unit does not fit one wavefront's LDS tile), a model whose bodies are not in
 * depth-first order.  n_frames = 0 or n_seq = 0 returns GMR_OK without a launch.  Asynchronous on in->stream; the handle's device
 * is selected.
 * A model without a hinge (a floating base alone, nq = 7) is answered, not refused: root_wrench, com, zmp and the ground-reaction
 * statistics are those of one rigid body; tau_out, armature, torque_limit and the per-hinge statistics are arrays of no columns,
 * may be NULL (a statistic then needs root_wrench_out only) and are not touched.
 * Layout (LP64): sizeof 272; offsets qpos 0, n_frames 8, seq_offsets 16, qvel 24, qacc 32, n_seq 40, nbody 44, fps 48,
 * gravity_x 56, gravity_y 64, gravity_z 72, ground_z 80, fz_min 88, body_parent 96, body_mass 104, body_com 112,
 * body_inertia 120, armature 128, torque_limit 136, stream 144, tau_out 152, root_wrench_out 160, com_out 168, zmp_out 176,
 * qvel_out 184, qacc_out 192, tau_abs_max_out 200, tau_rms_out 208, tau_ratio_max_out 216, frames_over_limit_out 224,
 * frames_any_over_limit_out 232, fz_ratio_max_out 240, fz_ratio_min_out 248, unloaded_frames_out 256,
 * nonfinite_frames_out 264.  */
typedef struct gmr_dynamics_input {
  const double  *qpos;            /* device [n_frames][nq] f64 */
  int64_t        n_frames;
  const int64_t *seq_offsets;     /* DEVICE [n_seq+1] */
  const double  *qvel, *qacc;     /* device [n_frames][nq-1] f64, or NULL = differences of qpos */
  int32_t        n_seq, nbody;    /* nbody: bodies of the inertial table */
  double         fps;
  double         gravity_x, gravity_y, gravity_z;
  double         ground_z, fz_min;
  const int32_t *body_parent;     /* device [nbody] */
  const double  *body_mass, *body_com, *body_inertia;   /* device [nbody], [nbody][3], [nbody][6] */
  const double  *armature, *torque_limit;               /* device [nq-7] */
  void          *stream;          /* the call's stream */
  double        *tau_out, *root_wrench_out, *com_out, *zmp_out;
  double        *qvel_out, *qacc_out;
  double        *tau_abs_max_out, *tau_rms_out, *tau_ratio_max_out;
  int32_t       *frames_over_limit_out, *frames_any_over_limit_out;
  double        *fz_ratio_max_out, *fz_ratio_min_out;
  int32_t       *unloaded_frames_out, *nonfinite_frames_out;
} gmr_dynamics_input;
int gmr_motion_dynamics(gmr_model *m, const gmr_dynamics_input *in);

/* Self-collision of retargeted qpos: per frame the smallest clearance over a list of capsule pairs, the pair that attains it and
 * the number of pairs in collision; per clip the deepest frame, its pair, and how many frames collide and for how long in a row.
 * A capsule is a segment fixed to a body plus a radius (a sphere when its ends coincide); which capsules and which pairs is the
 * caller's table (gmr_amd/collision.py builds a default from the kinematic tree -- not the robot's collision geometry).
 * All arithmetic is float64 without floating-point contraction, in the written order; a dot product u.v is (u_x v_x + u_y v_y) + u_z v_z.
 *
 * The whole call is this struct, its stream included (in->stream, in the sense of the stream-order paragraph at the top of this
 * file); the struct is read completely before the call returns.  The call enqueues two kernels on in->stream (one when no
 * statistic is asked for) and nothing else: no allocation, no copy, no synchronisation.  All arrays are device arrays.
 *   qpos          f64 [n_frames][nq], free-joint layout (x y z, qw qx qy qz, hinges), concatenated clips (N = n_frames)
 *   seq_offsets   int64 [n_seq+1]: clip s owns the rows a = clamp(seq_offsets[s], 0, N) to b = clamp(seq_offsets[s+1], a, N), T = b - a
 *                 (gmr_motion_dynamics' rule)
 *   cap_body      int32 [n_caps]: the body a capsule is fixed to.  Trusted; the kernel only clamps it into [0, nbody)
 *   cap_p0, cap_p1   f64 [n_caps][3]: the ends in the body frame.  Trusted
 *   cap_radius    f64 [n_caps].  Trusted
 *   pairs         int32 [n_pairs][2]: the capsule pairs (A, B) that are tested.  Trusted; the kernel only clamps into [0, n_caps)
 *   margin        a pair is a hit when its clearance is below margin (0: touching does not count)
 * Poses are gmr_motion_footlock's FK (MuJoCo's convention, the root quaternion divided by its norm), not the float32 gmr_fk.  With
 * x_j and the unit quaternion of body j, the world ends of capsule i on body j are P = x_j + R_j p0 and Q = x_j + R_j p1, R v
 * evaluated as t = 2 (u x v), v + w t + (u x t) for the quaternion (w, u).
 * Clearance of the pair (A, B) with ends (p1, q1) and (p2, q2):
 *   d1 = q1 - p1, d2 = q2 - p2, r = p1 - p2;  a = d1.d1, e = d2.d2, f = d2.r, c = d1.r, b = d1.d2, den = a e - b b
 *   s = den > 0 ? clamp01((b f - c e) / den) : 0;   t = e > 0 ? (b s + f) / e : 0
 *   if not e > 0 or t < 0:  t = 0, s = a > 0 ? clamp01(-c / a) : 0;   else if t > 1:  t = 1, s = a > 0 ? clamp01((b - c) / a) : 0
 *   (not e > 0: B is a sphere, and s is the point of A nearest its centre)
 *   w = (p1 + s d1) - (p2 + t d2);   clearance = sqrt(w.w) - (r_A + r_B)
 * clamp01(x) = x > 0 ? (x < 1 ? x : 1) : 0, which is 0 for a NaN.
 * Outputs per frame, any may be NULL:
 *   clearance_out [n_frames] f64   the minimum over the pairs; NaN when any pair's clearance is NaN (torch.min's rule, as the
 *                                  clip minimum of gmr_motion_contacts)
 *   pair_out [n_frames] i32        the lowest pair index that attains the minimum; -1 in a NaN frame
 *   hits_out [n_frames] i32        pairs with clearance < margin; 0 in a NaN frame
 * The minimum and its index are properties of the pair table: they do not depend on how the kernel spreads the pairs over its
 * lanes or the frames over its wavefronts.
 * Per-clip statistics, any may be NULL, reduced by the second kernel from the three per-frame outputs (all three are required when
 * a statistic is asked for).  Frames are counted from 0 at the clip's first row:
 *   clearance_min_out [n_seq] f64      the minimum over the clip's frames whose clearance is not NaN; +inf when there is none
 *   worst_frame_out [n_seq] i32        the earliest frame of the clip at that minimum; -1 when there is none (T < 2^31)
 *   worst_pair_out [n_seq] i32         that frame's pair_out; -1 when there is none
 *   colliding_frames_out [n_seq] i32   frames with hits > 0
 *   longest_run_out [n_seq] i32        the longest run of consecutive such frames (a NaN frame has no hits and ends a run)
 *   hits_sum_out [n_seq] i64           the sum of hits over the clip
 *   nonfinite_frames_out [n_seq] i32   frames whose clearance is NaN
 * A clip without frames reports +inf, -1, -1, 0, 0, 0, 0.  Rows outside every clip are not written.  Two calls give identical
 * bytes.  Non-finite input: a non-finite entry of a qpos row reaches only its own frame and its own clip's statistics; no byte of
 * another frame's outputs or another clip's statistics changes.  A zero root quaternion gives a NaN frame.
 * GMR_EINVAL: a non-finite margin, negative counts, and with work to do: n_caps < 1 or n_pairs < 1, NULL arrays, a statistic
 * without the three per-frame outputs.  GMR_EUNSUPPORTED: a model of more than 64 bodies (its poses do not fit one
 * wavefront's tile), a model in which a body precedes its parent, n_caps > 256, n_pairs > 32768.  n_frames = 0 or n_seq = 0
 * returns GMR_OK without a launch.  A planar-base model is accepted: internally it carries a free-joint qpos, and nothing here is
 * physics.  Asynchronous on in->stream; the handle's device is selected.
 * Layout (LP64): sizeof 176; offsets qpos 0, n_frames 8, seq_offsets 16, n_seq 24, n_caps 28, n_pairs 32, reserved 36,
 * cap_body 40, cap_p0 48, cap_p1 56, cap_radius 64, pairs 72, margin 80, stream 88, clearance_out 96, pair_out 104,
 * hits_out 112, clearance_min_out 120, worst_frame_out 128, worst_pair_out 136, colliding_frames_out 144,
 * longest_run_out 152, hits_sum_out 160, nonfinite_frames_out 168.  */
typedef struct gmr_self_collision_input {
  const double  *qpos;            /* device [n_frames][nq] f64 */
  int64_t        n_frames;
  const int64_t *seq_offsets;     /* DEVICE [n_seq+1] */
  int32_t        n_seq, n_caps;
  int32_t        n_pairs, reserved;
  const int32_t *cap_body;        /* device [n_caps] */
  const double  *cap_p0, *cap_p1, *cap_radius;   /* device [n_caps][3], [n_caps][3], [n_caps] */
  const int32_t *pairs;           /* device [n_pairs][2] */
  double         margin;
  void          *stream;          /* the call's stream */
  double        *clearance_out;
  int32_t       *pair_out, *hits_out;
  double        *clearance_min_out;
  int32_t       *worst_frame_out, *worst_pair_out, *colliding_frames_out, *longest_run_out;
  int64_t       *hits_sum_out;
  int32_t       *nonfinite_frames_out;
} gmr_self_collision_input;
int gmr_motion_self_collision(gmr_model *m, const gmr_self_collision_input *in);

/* Self-collision repair of retargeted qpos: every frame in which a capsule pair of gmr_motion_self_collision's tables comes closer
 * than margin is moved, over the hinges between the two capsules, until the pair is at the margin again -- a fixed number of
 * damped projection passes per frame, each frame on its own.  What gmr_motion_self_collision measures, this call removes; the
 * reference has no collision avoidance.  The defaults of the Python layers (16 passes, damping 1e-6 m^2, step_cap 0.2 rad,
 * resolve_tol 1e-4 m) are conventions, not measured on a robot.
 * All arithmetic is float64 without floating-point contraction, in the written order; a dot product u.v is (u_x v_x + u_y v_y) +
 * u_z v_z, a cross product a x b is (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x).
 *
 * The whole call is this struct, its stream included (in->stream, in the sense of the stream-order paragraph at the top of this
 * file); the struct is read completely before the call returns.  The call enqueues two kernels on in->stream (one when no
 * statistic is asked for) and nothing else: no allocation, no copy, no synchronisation.  All arrays are device arrays.
 *   qpos, n_frames, seq_offsets, n_seq, cap_body, cap_p0, cap_p1, cap_radius, pairs, n_caps, n_pairs, margin
 *                 as in gmr_self_collision_input, with its clamping rules (rows a .. b of clip s, cap_body into [0, nbody), pairs
 *                 into [0, n_caps)) and its FK (gmr_motion_footlock's: MuJoCo's convention, the root quaternion divided by its norm)
 *   iterations    I, 1 .. 32: the passes of a frame
 *   damping       lambda^2 > 0, in m^2
 *   step_cap      > 0, in rad: the largest change of a hinge in one pass
 *   resolve_tol   >= 0, in m: a frame whose clearance_after is below margin - resolve_tol counts as unresolved
 *   hinge_mask    by value; bit i set: hinge i, in qpos order (column 7 + i), may move
 * Definition, per frame of a clip, independently of every other frame.  A frame with a non-finite entry in its row is not
 * evaluated: its row is copied, clearance_before and clearance_after are NaN, move is 0.  Otherwise q0 is the row's own hinges,
 * q = q0, and the following pass runs exactly I times:
 *   1  the poses of all bodies at q (x_j, unit quaternion r_j), the capsule ends, and for every pair p = (A on body X, B on body Y)
 *      the report's s and t:  a_p = p1 + s d1,  b_p = p2 + t d2,  w = a_p - b_p,  nw = sqrt(w.w),  c_p = nw - (r_A + r_B)
 *   2  anc(b): the hinges on the path from the root to body b, b's own included.  M_p = (anc(X) xor anc(Y)) and hinge_mask.  (A
 *      shared ancestor moves both capsules rigidly and is left out by definition.  The root never moves.)
 *   3  v_p = margin - c_p when that is > 0 and M_p is not empty, else 0 (0 for a NaN).  V = sum_p v_p, pairs in ascending index
 *      from 0.0.  If V is not > 0, this pass and all later passes change nothing.
 *   4  n = w / nw when nw > 0, else 0
 *   5  hinge i on body j has the world axis u_i = rot(r_j, axis_j) and the anchor o_i = x_j.
 *        g_pi = n . (u_i x (a_p - o_i))      for i in M_p and anc(X)
 *        g_pi = -(n . (u_i x (b_p - o_i)))   for i in M_p and anc(Y)
 *        g_pi = 0                            elsewhere
 *      (the exact derivative of nw with the closest-point parameters s, t held fixed)
 *   6  rho_p = v_p / (sum_i g_pi g_pi + lambda^2), hinges in ascending qpos order from 0.0;
 *      dq_i = (sum_p (v_p rho_p) g_pi) / V, pairs in ascending index from 0.0.  (A simultaneous projection with the weights v_p / V,
 *      which are continuous in the pose; a single colliding pair is moved exactly to the margin of its linearisation.)
 *   7  m = max_i |dq_i|, scale = m > step_cap ? step_cap / m : 1;  for every hinge of hinge_mask with dq_i != 0:
 *      q_i = clamp(q_i + scale dq_i, min(lo_i, q0_i), max(hi_i, q0_i)) for a limited hinge, unclamped otherwise (gmr_motion_footlock's
 *      rule); a hinge with dq_i = 0 keeps its bits.
 * After the last pass the clearances are evaluated once more at the final q.  The order of the two sums is part of the definition;
 * how the kernel forms them is its own business and results agree with the definition to rounding (as gmr_motion_dynamics').
 * Nothing in the map is a discrete choice except v_p > 0, whose contribution vanishes at the threshold: the map is continuous in
 * the row.  A pair whose segments' axes cross (nw = 0) has no normal and is not moved.
 * Outputs, device arrays:
 *   qpos_out [n_frames][nq] f64         required, must not alias qpos.  The rows with the final hinges.  Every other entry -- the
 *                                       root's seven, hinges outside hinge_mask, frames with V = 0 in the first pass, frames with a
 *                                       non-finite entry -- is copied bit for bit
 *   clearance_before_out [n_frames] f64 the minimum of c_p over all pairs at q0; NaN when any c_p is NaN (the report's rule: a zero
 *                                       root quaternion gives a NaN frame) and in a frame with a non-finite entry.  May be NULL
 *   clearance_after_out [n_frames] f64  the same at the final q.  May be NULL
 *   move_out [n_frames] f64             max_i |q_i - q0_i| over the hinges, 0 without one.  May be NULL
 * Per-clip statistics, any may be NULL, reduced by the second kernel from the three per-frame arrays (all three are required when
 * a statistic is asked for).  A frame whose clearance_after is NaN is counted in nonfinite_frames and takes part in no other
 * statistic:
 *   repaired_frames_out [n_seq] i32       frames with move > 0
 *   unresolved_frames_out [n_seq] i32     frames with clearance_after < margin - resolve_tol
 *   move_max_out [n_seq] f64              the maximum of move, 0 without a frame
 *   clearance_min_after_out [n_seq] f64   the minimum of clearance_after; +inf for a clip without a finite frame
 *   nonfinite_frames_out [n_seq] i32
 * A clip without frames reports 0, 0, 0, +inf, 0.  Rows outside every clip are not written.  Two calls give identical bytes.
 * Non-finite input reaches only its own frame and its own clip's statistics.
 * GMR_EINVAL: I outside 1 .. 32, damping or step_cap not finite and > 0, a negative or non-finite resolve_tol, a non-finite margin,
 * qpos_out == qpos, negative counts, and with work to do: NULL arrays, a statistic without the three per-frame arrays, n_caps < 1
 * or n_pairs < 1.  GMR_EUNSUPPORTED: a model of more than 64 bodies (and with them more than 64 hinges: a hinge is a body's), a
 * model in which a body precedes its parent, n_caps > 256, n_pairs > 32768, a planar-base model (a planar-base qpos the caller
 * holds is not in free-joint layout).  These are checked before anything is enqueued.  n_frames = 0 or n_seq = 0 returns GMR_OK
 * without a launch.  Asynchronous on in->stream; the handle's device is selected.
 * Layout (LP64): sizeof 200; offsets qpos 0, n_frames 8, seq_offsets 16, n_seq 24, n_caps 28, n_pairs 32, iterations 36,
 * cap_body 40, cap_p0 48, cap_p1 56, cap_radius 64, pairs 72, margin 80, damping 88, step_cap 96, resolve_tol 104,
 * hinge_mask 112, stream 120, qpos_out 128, clearance_before_out 136, clearance_after_out 144, move_out 152,
 * repaired_frames_out 160, unresolved_frames_out 168, move_max_out 176, clearance_min_after_out 184,
 * nonfinite_frames_out 192.  */
typedef struct gmr_self_collision_repair_input {
  const double  *qpos;            /* device [n_frames][nq] f64 */
  int64_t        n_frames;
  const int64_t *seq_offsets;     /* DEVICE [n_seq+1] */
  int32_t        n_seq, n_caps;
  int32_t        n_pairs, iterations;
  const int32_t *cap_body;        /* device [n_caps] */
  const double  *cap_p0, *cap_p1, *cap_radius;   /* device [n_caps][3], [n_caps][3], [n_caps] */
  const int32_t *pairs;           /* device [n_pairs][2] */
  double         margin, damping, step_cap, resolve_tol;
  uint64_t       hinge_mask;      /* bit i: hinge i (qpos column 7 + i) may move */
  void          *stream;          /* the call's stream */
  double        *qpos_out;
  double        *clearance_before_out, *clearance_after_out, *move_out;
  int32_t       *repaired_frames_out, *unresolved_frames_out;
  double        *move_max_out, *clearance_min_after_out;
  int32_t       *nonfinite_frames_out;
} gmr_self_collision_repair_input;
int gmr_motion_self_collision_repair(gmr_model *m, const gmr_self_collision_repair_input *in);

/* The left-right mirrored copy of retargeted qpos: every row's hinge columns permuted with signs, its root reflected.  Which
 * column is the image of which is the caller's table (gmr_amd/symmetry.py derives it from the kinematic tree and refuses a
 * robot that is not symmetric); the entry does not judge it.
 *
 * The whole call is this struct, its stream included (in->stream, in the sense of the stream-order paragraph at the top of this
 * file); the struct is read completely before the call returns.  The call enqueues one kernel on in->stream and nothing else: no
 * allocation, no copy, no synchronisation, no scratch.  All arrays are device arrays; loads and stores are element-wise, so every
 * array needs the alignment of its element type only.
 *   qpos          f64 [n_frames][nq], free-joint layout (x y z, qw qx qy qz, hinges), concatenated clips (N = n_frames)
 *   seq_offsets   int64 [n_seq+1]: clip s owns the rows a = clamp(seq_offsets[s], 0, N) to b = clamp(seq_offsets[s+1], a, N), T = b - a
 *                 (gmr_motion_dynamics' rule).  Clips are expected not to overlap
 *   col_src       int32 [nq], col_sign f64 [nq]: only the elements 7 .. nq-1 are read.  Trusted: the caller guarantees
 *                 7 <= col_src[c] < nq (gmr_amd.symmetry.SymmetryPlan checks it, and that the map is an involution, before the
 *                 Python layer uploads a table); the kernel only clamps col_src[c] into [7, nq-1] and reads no more of col_sign[c]
 *                 than whether it is < 0
 *   mode          GMR_MIRROR_WORLD or GMR_MIRROR_CLIP_START
 *   qpos_out      f64 [n_frames][nq], not qpos: a row is permuted, so the call cannot work in place
 * Per row q with root position p = q[0:3] and root quaternion r = q[3:7] (w x y z):
 *   hinges, both modes:  out[c] = q[col_src[c]] for c >= 7, negated when col_sign[c] < 0.  A copy and a sign flip: with
 *   col_sign[c] = +-1 this is col_sign[c] * q[col_src[c]], and no arithmetic touches the value (a NaN keeps its payload).
 *   GMR_MIRROR_WORLD (0), the reflection in the world plane y = 0:  p' = (p_x, -p_y, p_z),  r' = (w, -x, y, -z).  The whole call is
 *   copies and sign flips: the output is bit-exact against this definition, and with a table that is an involution mirroring
 *   twice returns the input bytes (a negation flips the sign bit, so -0.0 comes back as -0.0 too).
 *   GMR_MIRROR_CLIP_START (1), the reflection of each clip in the vertical plane through its first row's root position p0 along
 *   that row's heading, so that the mirrored clip starts where the original started, facing the same way.  With the first row's
 *   root (p0, r0), f = R(r0 / |r0|) e_x and the heading psi = atan2(f_y, f_x):
 *     p'_xy = p0_xy + [[cos 2psi, sin 2psi], [sin 2psi, -cos 2psi]] (p - p0)_xy,  p'_z = p_z (a copy)
 *     r'    = r_z(2 psi) (x) (w, -x, y, -z),  r_z(2 psi) = (cos psi, 0, 0, sin psi)
 *   psi = 0 when f_x^2 + f_y^2 < 1e-12: a convention for a root that points straight up, where the heading is not defined.
 *   The map is linear in r, so sign continuity and the norm carry over; nothing is normalised.  No trigonometric function is
 *   evaluated.  All arithmetic is float64 without floating-point contraction, in this order:
 *     n = sqrt(((w0 w0 + x0 x0) + y0 y0) + z0 z0);  (w, x, y, z) = r0 / n, element-wise
 *     f_x = 1 - 2 (y y + z z);  f_y = 2 (x y + w z);  h2 = f_x f_x + f_y f_y
 *     h2 < 1e-12:  cp = 1, sp = 0, c2 = 1, s2 = 0;   otherwise  h = sqrt(h2), cp = f_x / h, sp = f_y / h,
 *                  c2 = (f_x f_x - f_y f_y) / h2, s2 = (2 f_x f_y) / h2      (cos psi, sin psi, cos 2psi, sin 2psi)
 *     d = p - p0:  p'_x = p0_x + (c2 d_x + s2 d_y),  p'_y = p0_y + ((-c2) d_y + s2 d_x)
 *     r'_w = cp w + sp z,  r'_x = (-cp) x + (-sp) y,  r'_y = cp y + (-sp) x,  r'_z = (-cp) z + sp w       (of the row's r)
 * Rows outside every clip are not written.  A clip without frames does no work.  Two calls give identical bytes.
 * Non-finite input: in GMR_MIRROR_WORLD a non-finite entry reaches exactly the output element it is copied to.  In
 * GMR_MIRROR_CLIP_START a non-finite root entry of a clip's first row reaches root columns of that clip's rows only, a non-finite
 * root entry of another row reaches root columns of that row only.  Hinge columns are never affected by the root, and no other
 * clip changes, in either mode.
 * GMR_EINVAL: negative counts, an unknown mode, and with work to do: NULL arrays, qpos_out == qpos.  GMR_EUNSUPPORTED: nq > 64 (a
 * row does not fit one wavefront), a planar-base model.  n_frames = 0 or n_seq = 0 returns GMR_OK without a launch.
 * Asynchronous on in->stream; the handle's device is selected.
 * Layout (LP64): sizeof 72; offsets qpos 0, n_frames 8, seq_offsets 16, n_seq 24, mode 28, col_src 32, col_sign 40, stream 48,
 * qpos_out 56, reserved 64.  */
#define GMR_MIRROR_WORLD 0
#define GMR_MIRROR_CLIP_START 1
typedef struct gmr_mirror_input {
  const double  *qpos;            /* device [n_frames][nq] f64 */
  int64_t        n_frames;
  const int64_t *seq_offsets;     /* DEVICE [n_seq+1] */
  int32_t        n_seq, mode;
  const int32_t *col_src;         /* device [nq] */
  const double  *col_sign;        /* device [nq] */
  void          *stream;          /* the call's stream */
  double        *qpos_out;        /* device [n_frames][nq] f64, not qpos */
  int64_t        reserved;        /* 0 */
} gmr_mirror_input;
int gmr_motion_mirror(gmr_model *m, const gmr_mirror_input *in);

/* Composed clips: long reference motions made of segments of the source clips, each segment moved by a planar rigid map onto the
 * end of the one before it and cross-faded into it over the frames they share.  What a trainer needs for references longer than
 * a capture take (walk -> turn -> run, a cycle repeated) and for transitions that do not teleport the robot.  The result is
 * ordinary qpos: it feeds gmr_motion_footlock (which removes the slide a cross-fade puts into planted feet), gmr_motion_track
 * and the reports unchanged.  Which segments follow which is the caller's plan (gmr_amd/compose.py builds and checks it); the
 * entry does not judge it.
 *
 * The whole call is this struct, its stream included (in->stream, in the sense of the stream-order paragraph at the top of this
 * file); the struct is read completely before the call returns.  The call enqueues two kernels on in->stream and nothing else: no
 * allocation, no copy, no synchronisation, no hidden scratch (seg_transform is the hand-over between the two kernels).  All
 * arrays are device arrays; loads and stores are element-wise, so every array needs the alignment of its element type only.
 *   qpos          f64 [n_frames][nq], free-joint layout (x y z, qw qx qy qz, hinges).  The plan addresses absolute rows, so the
 *                 clips' seq_offsets are not needed here
 *   seg_src       int64 [n_seg]: the absolute source row of segment k's first frame
 *   seg_len       int32 [n_seg]: its frames, at least 1
 *   seg_blend     int32 [n_seg]: the frames it overlaps with the segment before it in the same output clip: 0 exactly for the first
 *                 segment of an output clip, at least 1 for every other
 *   seg_out       int64 [n_seg]: the absolute output row of its first frame, seg_out[k] = seg_out[k-1] + seg_len[k-1] - seg_blend[k]
 *   clip_segs     int64 [n_out+1]: output clip o is the chain of the segments clip_segs[o] .. clip_segs[o+1]-1 (none: an empty clip)
 *   qpos_out      f64 [n_out_frames][nq], not qpos
 *   seg_transform f64 [n_seg][6] = (c, s, tx, ty, hw, hz): where each segment was placed.  A result, and what the second kernel reads
 * Plan invariants: seg_blend[k] <= seg_len[k-1], and seg_blend[k] + seg_blend[k+1] <= seg_len[k], so every output row reads at
 * most two source rows.  Segment k writes the output rows seg_out[k] + j, 0 <= j < seg_len[k] - seg_blend[k+1], where
 * seg_blend[k+1] counts as 0 for the last segment of an output clip.  The tables are trusted as gmr_mirror_input's col_src is
 * (gmr_amd.compose.ComposePlan checks every invariant before the Python layer uploads a table): the kernels only clamp source
 * rows into [0, n_frames-1] and segment indices into [0, n_seg], and drop output rows outside [0, n_out_frames), so that a wrong
 * table cannot leave the arrays.
 *
 * Placement.  Segment k has a planar rigid map T_k = (c_k, s_k, tx_k, ty_k) and a half-angle quaternion (hw_k, 0, 0, hz_k).  A
 * row with root position p and root quaternion r (w x y z) is placed as
 *   p'_x = (c p_x - s p_y) + tx,  p'_y = (s p_x + c p_y) + ty,  p'_z = p_z (a copy)
 *   r'   = (hw, 0, 0, hz) (x) r:  r'_w = hw w - hz z,  r'_x = hw x - hz y,  r'_y = hw y + hz x,  r'_z = hw z + hz w
 * which is linear in r: nothing is normalised.  Hinges are untouched.  The first segment of an output clip has the identity
 * (1, 0, 0, 0, 1, 0) and its rows are used without arithmetic: outside an overlap they are copied bit for bit.
 * For any other segment, with B = seg_blend[k], the anchor is a = B / 2 (integer division) and the anchor pair is the previous
 * segment's source row A = seg_src[k-1] + seg_len[k-1] - B + a and this segment's row Bk = seg_src[k] + a.  The heading of a row
 * is the mirror contract's: n = sqrt(((w w + x x) + y y) + z z), (w, x, y, z) = r / n, f_x = 1 - 2 (y y + z z),
 * f_y = 2 (x y + w z), h2 = f_x f_x + f_y f_y;  h2 < 1e-12: (cos, sin) = (1, 0) (a root pointing straight up);  otherwise
 * h = sqrt(h2), (cos, sin) = (f_x / h, f_y / h).  No trigonometric function is evaluated.  With (ca, sa) of row A and (cb, sb) of
 * row Bk the relative map D_k turns this segment's anchor heading and xy onto the previous segment's:
 *   cd = ca cb + sa sb,  sd = sa cb - ca sb,  tdx = pa_x - (cd pb_x - sd pb_y),  tdy = pa_y - (sd pb_x + cd pb_y)
 * and T_k = T_{k-1} o D_k, composed sequentially in segment order (c, s, tx, ty, hw, hz of segment k-1 on the right-hand sides):
 *   nx = (c tdx - s tdy) + tx,  ny = (s tdx + c tdy) + ty,  c1 = c cd - s sd,  s1 = s cd + c sd,  n = sqrt(c1 c1 + s1 s1)
 *   c_k = c1 / n,  s_k = s1 / n,  tx_k = nx,  ty_k = ny
 * The half angle, without a trigonometric function, hw >= 0 in both branches:
 *   c_k < 0:   m = sqrt((1 - c_k) 0.5),  hw = |s_k| / (2 m),  hz = -m if s_k < 0, else m      (a turn of pi: (0, +-1) to rounding)
 *   otherwise: hw = sqrt((1 + c_k) 0.5),  hz = s_k / (2 hw)
 * Then the sign: with qa = (hw_{k-1}, 0, 0, hz_{k-1}) (x) r_A and qb = (hw, 0, 0, hz) (x) r_Bk, if
 * ((qa_w qb_w + qa_x qb_x) + qa_y qb_y) + qa_z qb_z < 0 then (hw_k, hz_k) = (-hw, -hz).  So the placed quaternions of the two
 * segments have a non-negative dot product at the anchor row: sign continuity across a transition is guaranteed there.  In the
 * rest of the overlap the slerp below takes the shortest arc, whichever signs its two rows have.
 *
 * Blend.  Row j < B of segment k combines the previous segment's frame seg_len[k-1] - B + j placed by T_{k-1} (x0) and this
 * segment's frame j placed by T_k (x1):  u = (j + 1) / (B + 1),  w = (u u) (3 - 2 u), never 0 or 1 (no frame of the overlap is
 * wasted).  Root xy, root z (the raw values) and every hinge: x0 + w (x1 - x0).  Root quaternion: the shortest-arc slerp of the
 * two placed quaternions at w, normalised (the tracking export's: acos, sin).  Row j >= B is this segment's own, placed.
 * All arithmetic is float64 without floating-point contraction, in the order written here.  Two calls give identical bytes.
 *
 * Non-finite input: a non-finite hinge entry reaches only the output rows that read its row, in that column.  A non-finite root
 * entry of a row that is no anchor reaches root columns of the output rows that read it.  A non-finite root entry of an anchor
 * row reaches root columns of that segment (for row A: of the next one) and of the later segments of the same output clip.  No
 * other output clip changes, and no hinge column is affected by a root.
 * GMR_EINVAL: negative counts, and with work to do: NULL arrays, n_frames = 0, qpos_out == qpos.  GMR_EUNSUPPORTED: nq > 64 (a
 * row does not fit one wavefront), a planar-base model.  n_seg = 0, n_out = 0 or n_out_frames = 0 returns GMR_OK without a launch.
 * Asynchronous on in->stream; the handle's device is selected.
 * Layout (LP64): sizeof 104; offsets qpos 0, n_frames 8, seg_src 16, seg_len 24, seg_blend 32, seg_out 40, clip_segs 48, n_seg 56,
 * n_out 60, n_out_frames 64, stream 72, qpos_out 80, seg_transform 88, reserved 96.  */
typedef struct gmr_compose_input {
  const double  *qpos;            /* device [n_frames][nq] f64 */
  int64_t        n_frames;
  const int64_t *seg_src;         /* device [n_seg] */
  const int32_t *seg_len;         /* device [n_seg] */
  const int32_t *seg_blend;       /* device [n_seg] */
  const int64_t *seg_out;         /* device [n_seg] */
  const int64_t *clip_segs;       /* device [n_out+1] */
  int32_t        n_seg, n_out;
  int64_t        n_out_frames;
  void          *stream;          /* the call's stream */
  double        *qpos_out;        /* device [n_out_frames][nq] f64, not qpos */
  double        *seg_transform;   /* device [n_seg][6] f64 */
  int64_t        reserved;        /* 0 */
} gmr_compose_input;
int gmr_motion_compose(gmr_model *m, const gmr_compose_input *in);

/* Transition search: for windows of L frames of the clips, the motion-graph distance of Kovar, Gleicher and Pighin (2002) -- the
 * weighted squared distance of two windows of body positions after the best rotation about z and shift in xy of one of them -- for
 * every source frame against every frame of every target clip, reduced where it is computed to the best target frame per (source
 * frame, target clip).  What a caller needs in front of gmr_motion_compose to choose which frame of which clip follows which
 * (gmr_amd/transitions.py turns the result into transitions and into plans for gmr_amd.compose.ComposePlan).
 *
 * The whole call is this struct, its stream included (in->stream, in the sense of the stream-order paragraph at the top of this
 * file); the struct is read completely before the call returns.  The call enqueues three kernels on in->stream and nothing else: no
 * allocation, no copy, no synchronisation, no hidden scratch (points and moments are the hand-over between the kernels, and
 * results).  All arrays are device arrays; loads and stores are element-wise, so every array needs the alignment of its element
 * type only.
 *   qpos          f64 [n_frames][nq], free-joint layout (x y z, qw qx qy qz, hinges), concatenated clips (N = n_frames)
 *   seq_offsets   int64 [n_seq+1]: clip s owns the rows a = clamp(seq_offsets[s], 0, N) to b = clamp(seq_offsets[s+1], a, N), T = b - a
 *                 (gmr_motion_dynamics' rule; T < 2^30).  Clips are expected not to overlap
 *   body_ids      int32 [n_bodies]: point p lies on body body_ids[p] (its frame origin).  Trusted; the kernel only clamps into [0, nbody)
 *   weights       f64 [n_bodies]: w_p >= 0.  The caller normalises them to sum 1; the kernels use them as given
 *   window        L >= 1 frames, uniform frame weights; src_stride s >= 1; min_gap >= 0
 *   src_clips     int32 [n_src_clips], dst_clips int32 [n_dst_clips]: clips of seq_offsets.  Trusted; clamped into [0, n_seq)
 *   src_offsets   int64 [n_src_clips+1]: source clip a owns the sources src_offsets[a] .. src_offsets[a+1]-1, source u of it being the
 *                 frame i = u s of the clip: the frames 0, s, 2s, ... <= T_A - L, none for a clip shorter than L.  From 0, ascending,
 *                 to n_sources = E.  Trusted; a source the clip does not have reports +inf and -1
 *   dst_offsets   int64 [n_dst_clips+1]: target clip b owns the columns dst_offsets[b] + j of cost_out, j = 0 .. T_B - L: every frame
 *                 that starts a full window, stride 1; to n_targets.  Read only when cost_out is given
 * Points.  x[f][p] in R^3 is the position of body body_ids[p] in row f: gmr_motion_footlock's FK in float64 (MuJoCo's convention, the
 * root quaternion divided by its norm), exactly as gmr_motion_self_collision evaluates poses; then the clip's first-row root (x, y)
 * -- qpos columns 0 and 1 of its first row -- is subtracted from x and y of every row of that clip (z is kept), so that magnitudes
 * stay at the clip's own extent and the cost does not depend on where the clip lies.
 *   points        f64 [n_frames][n_bodies][3], written for every row of every clip of seq_offsets.  Scratch and a result
 *   moments       f64 [n_frames][6] = (m.x, m.y, q, M.x, M.y, V).  Scratch and a result; the last three only for rows that start a
 *                 full window of their clip
 * All sums start from 0 and add their terms in ascending order, s = s + term.  Per row, over p:
 *   m_f = sum w_p (x, y)            terms w_p x and w_p y
 *   q_f = sum w_p (x x + y y)
 * Per pair of rows (f of the source clip, g of the target clip), over p:
 *   Gd(f,g) = sum w_p (x_f x_g + y_f y_g)
 *   Gc(f,g) = sum w_p (x_f y_g - y_f x_g)
 *   Gz(f,g) = sum w_p ((z_f - z_g) (z_f - z_g))
 * Per window, sums over k = 0 .. L-1, then one division by L (the double of L):
 *   M_i = (sum m_{i+k}) / L per component,  Q_i = (sum q_{i+k}) / L,  V_i = Q_i - (M_i.x M_i.x + M_i.y M_i.y)
 *   D(i,j) = (sum Gd(i+k, j+k)) / L - (M_i.x M_j.x + M_i.y M_j.y)
 *   C(i,j) = (sum Gc(i+k, j+k)) / L - (M_i.x M_j.y - M_i.y M_j.x)
 *   Z(i,j) = (sum Gz(i+k, j+k)) / L
 *   cost(i,j) = ((V_i + V_j) - 2 sqrt(D D + C C)) + Z;   a cost < 0 is replaced by 0, a NaN stays a NaN
 * which is the minimum over a rotation R about z and a shift t in xy of  mean_k sum_p w_p |a_{i+k,p} - (R b_{j+k,p} + t)|^2  for
 * weights that sum to 1 (a the source's points, b the target's); the best rotation has (cos, sin) proportional to (D, -C).
 * Float64, no floating-point contraction, IEEE sqrt and division, the operations in the order written: given the same points a
 * numpy restatement equals the kernels bit for bit.
 * In a composition, pair (i, j) is the overlap of Segment(A, a0, i + L - a0) followed by Segment(B, j, n) with blend = L: rows
 * A[i+k] are cross-faded with B[j+k].
 * Exclusion: where src_clips[a] == dst_clips[b] (after clamping), the pairs with |j - i| < min_gap are excluded; min_gap = 0
 * excludes nothing.
 * Outputs:
 *   best_cost     f64 [E][n_dst_clips]: the minimum over the target clip's frames that are not excluded and whose cost is not NaN
 *   best_frame    i32 [E][n_dst_clips]: the lowest frame j at that minimum, counted from the clip's first row;  +inf and -1 when
 *                 there is no such frame
 *   cost_out      f64 [E][n_targets], may be NULL: the dense matrix, for small inputs, plots and tests; an excluded pair is +inf
 * Two calls give identical bytes, and no output depends on how the pairs are spread over lanes, wavefronts or workgroups
 * (GMR_AMD_TRANSITIONS_WAVES and GMR_AMD_TRANSITIONS_TILE force the launch geometry).  Non-finite input: a non-finite entry of a
 * qpos row reaches the points and (m, q) of that row, the (M, V) of the windows that contain it, and the pairs whose windows contain
 * it; a non-finite root (x, y) of a clip's first row reaches every row of that clip; no other output byte changes.
 * GMR_EINVAL: window < 1, src_stride < 1, n_bodies < 1, min_gap < 0, negative counts, and with work to do: NULL arrays (cost_out
 * without dst_offsets included).  GMR_EUNSUPPORTED: a model of more than 64 bodies, a model in which a body precedes its parent
 * (as gmr_motion_self_collision), n_bodies > 64, window > 32 (the windowed sums live in a register ring).  n_frames = 0,
 * n_seq = 0, n_src_clips = 0, n_dst_clips = 0 or n_sources = 0 returns GMR_OK without a launch.  A planar-base model is accepted, as
 * in gmr_motion_self_collision.  Asynchronous on in->stream; the handle's device is selected.
 * Layout (LP64): sizeof 168; offsets qpos 0, n_frames 8, seq_offsets 16, n_seq 24, n_bodies 28, body_ids 32, weights 40, window 48,
 * src_stride 52, min_gap 56, n_src_clips 60, n_dst_clips 64, reserved 68, src_clips 72, src_offsets 80, dst_clips 88,
 * dst_offsets 96, n_sources 104, n_targets 112, stream 120, points 128, moments 136, best_cost 144, best_frame 152, cost_out 160.  */
typedef struct gmr_transitions_input {
  const double  *qpos;            /* device [n_frames][nq] f64 */
  int64_t        n_frames;
  const int64_t *seq_offsets;     /* DEVICE [n_seq+1] */
  int32_t        n_seq, n_bodies;
  const int32_t *body_ids;        /* device [n_bodies] */
  const double  *weights;         /* device [n_bodies] */
  int32_t        window, src_stride;
  int32_t        min_gap, n_src_clips;
  int32_t        n_dst_clips, reserved;
  const int32_t *src_clips;       /* device [n_src_clips] */
  const int64_t *src_offsets;     /* device [n_src_clips+1] */
  const int32_t *dst_clips;       /* device [n_dst_clips] */
  const int64_t *dst_offsets;     /* device [n_dst_clips+1], for cost_out */
  int64_t        n_sources;       /* E = src_offsets[n_src_clips] */
  int64_t        n_targets;       /* dst_offsets[n_dst_clips] */
  void          *stream;          /* the call's stream */
  double        *points;          /* device [n_frames][n_bodies][3] f64 */
  double        *moments;         /* device [n_frames][6] f64 */
  double        *best_cost;       /* device [E][n_dst_clips] f64 */
  int32_t       *best_frame;      /* device [E][n_dst_clips] i32 */
  double        *cost_out;        /* device [E][n_targets] f64, or NULL */
} gmr_transitions_input;
int gmr_motion_transitions(gmr_model *m, const gmr_transitions_input *in);

/* Retiming to joint velocity limits: every clip played slower exactly where a hinge turns faster than its limit, by a monotone time
 * warp, and resampled along the warp at the clip's own rate.  The joint-space path is kept -- the remedy for a kick or a fall
 * recovery whose hinges outrun the actuators that neither drops the clip nor lets the pose fall behind its key-points (a velocity
 * limit inside the IK solve does).  The result is ordinary qpos with its own clip offsets: it feeds gmr_motion_footlock,
 * gmr_motion_track, gmr_motion_dynamics, gmr_motion_sample and gmr_motion_compose unchanged.
 *
 * Two entries, because the output length depends on the data: gmr_motion_retime_plan writes the warp and every clip's output
 * length, the caller turns the lengths into out_offsets (a prefix sum; reading them back is the one host synchronisation of the
 * pair, and the caller's) and allocates, gmr_motion_retime_apply resamples.  For each entry the whole call is its struct, the
 * stream included (in->stream, in the sense of the stream-order paragraph at the top of this file); the struct is read completely
 * before the call returns.  A call enqueues its kernels on in->stream (plan: three, apply: one) and nothing else: no allocation, no
 * copy, no synchronisation, no hidden scratch -- need, ticks and cum are the hand-over between the kernels and between the two
 * entries, and results.  All arrays are device arrays; loads and stores are element-wise, so every array needs the alignment of
 * its element type only.
 *
 * Time is an integer: Q = 1024 ticks per source frame.  The per-clip sums are exact in any order, and two calls give identical
 * bytes.
 *
 * gmr_motion_retime_plan
 *   qpos          f64 [n_frames][nq], free-joint layout (x y z, qw qx qy qz, hinges), concatenated clips (N = n_frames)
 *   seq_offsets   int64 [n_seq+1]: clip s owns the rows a = clamp(seq_offsets[s], 0, N) to b = clamp(seq_offsets[s+1], a, N), n = b - a
 *                 (gmr_motion_dynamics' rule).  Clips are expected not to overlap
 *   fps           the clips' rate, one per call, finite and > 0
 *   vmax          f64 [nq-7], rad/s per hinge in qpos order, every entry > 0; +inf: no limit.  Trusted (the Python layer checks it)
 *   window        W in [0, 32] intervals;  max_stretch in [1, 64]
 * A clip of n rows has n - 1 intervals; interval i lies between its rows i and i + 1 and its values are stored at row i.  The last
 * row of every clip gets need = 0 and ticks = 0.  All arithmetic is float64 without floating-point contraction, in the order
 * written:
 *   need_ij = (fabs(q[i+1][7+j] - q[i][7+j]) * fps) / vmax[j]     per hinge j
 *   the interval is NON-FINITE when any need_ij is not < +inf (a NaN or an infinity): then need_i = NaN (0x7ff8000000000000), it
 *   stretches as 1, and it is counted;  otherwise need_i = max_j need_ij, 0 for a model without hinges.  The root columns do not
 *   enter: a floating base has no actuator, and its speed scales with the warp anyway
 *   s_i = min(max(1, need_i), max_stretch)      a clip is never sped up;  the interval is CAPPED when need_i > max_stretch
 *   d_i = max of s_k over the intervals k in [i-W, i+W] of the clip
 *   m_i = (the sum of d_k over the same k, in ascending k, starting from the first d_k) / (double)(their number)
 *         every d_k of the window is at least s_i, so m_i >= s_i: the warp never undercuts a limit (where nothing is capped),
 *         and the stretch changes by at most (max_stretch - 1) / (2W + 1) per frame
 *   ticks_i = (int64)ceil(m_i * 1024.0)
 *   cum[row] = the sum of ticks of the clip's earlier intervals: 0 in its first row, total in its last
 *   out_len = 0 for a clip without rows, else (total + Q - 1) / Q + 1
 *   need          f64 [n_frames];  ticks, cum  int64 [n_frames];  rows outside every clip are not written
 *   out_len       int64 [n_seq]
 *   clip_stats    int64 [n_seq][4] = (intervals with need_i > 1, capped intervals, non-finite intervals, total)
 *   need_max      f64 [n_seq]: the largest finite need_i, 0 when there is none
 * Clips of less than 2^31 rows.
 *
 * gmr_motion_retime_apply
 *   qpos, seq_offsets, ticks, cum   as above: ticks and cum as gmr_motion_retime_plan wrote them for these clips
 *   out_offsets   int64 [n_seq+1]: clip s owns the output rows out_offsets[s] .. out_offsets[s+1]-1, clamped into
 *                 [0, n_out_frames] as seq_offsets is.  The caller builds it from out_len
 *   qpos_out      f64 [n_out_frames][nq], not qpos;  src_time  f64 [n_out_frames]
 * Output row k of a clip with n >= 1 rows is sampled at tau = k Q:
 *   tau >= total: a bit-for-bit copy of the clip's last row, src_time = n - 1.  So the clip ends in its exact final pose, and the
 *   last output interval only runs slower than planned
 *   otherwise: the interval i with cum[i] <= tau < cum[i+1], u = (double)(tau - cum[i]) / (double)ticks[i], src_time = i + u (it
 *   lets a caller warp per-frame labels such as contacts alongside the qpos).  Root position and hinges: x0 if u == 0, else
 *   x0 + u (x1 - x0) (the tracking export's lerp).  Root quaternion: a copy of row i's if u == 0 or if the two rows' quaternions
 *   are bytewise equal, otherwise the tracking export's shortest-arc slerp of the two at u, normalised, w x y z as stored
 * interp = GMR_RETIME_INTERP_CUBIC (1; 0 is the linear resampling above, any other value GMR_EINVAL) changes what a row with u != 0
 * holds and nothing else -- the search, src_time, the bitwise copy of row i at u == 0 and of the last row at tau >= total,
 * truncation and clamping are the same.  A linearly resampled path has all its acceleration at the source rows; the cubic is C1,
 * which is what retiming to TORQUE limits needs (below).  Per column, in float64 without contraction, in the order written:
 *   p1 = row i, p2 = row i+1;  p0 = row i-1, or p1 + (p1 - p2) when i = 0;  p3 = row i+2, or p2 + (p2 - p1) when i+2 is past the clip
 *   m1 = 0.5 (p2 - p0),  m2 = 0.5 (p3 - p1),  c = p2 - p1                     (Catmull-Rom tangents)
 *   y  = p1 + u (m1 + u (((3 c - 2 m1) - m2) + u ((m1 + m2) - 2 c)))
 *   Root quaternion: the stored rows p0, p2 and p3 are negated where their dot product with p1 (((w w' + x x') + y y') + z z') is
 *   negative -- before any reflection -- the same cubic runs per component, and the result is divided by its norm (the square root
 *   of ((w w + x x) + y y) + z z, four quotients).
 *   A clip of two rows gives the lerp to rounding.  A cubic may overshoot a joint range and, by a little, the velocity limit the plan
 *   was made for; the clip report (gmr_clip_report) of the result shows it.  A non-finite qpos entry reaches the output rows whose
 *   four-row stencil reads it, in its column -- in the quaternion all four components -- and nothing else.
 * A clip given fewer output rows than out_len is truncated; one given more repeats its last row; a clip without rows writes
 * nothing.  Row and interval indices are clamped into the clip (the search looks only at intervals 0 .. min(k, n-2)), so a wrong
 * out_offsets, ticks or cum cannot leave the arrays.
 *
 * Non-finite qpos.  A non-finite hinge entry reaches only the output rows that interpolate its row (u != 0 next to it, or a copy
 * of it), in that column; it makes its two intervals non-finite: their need is NaN and they stretch as 1, so ticks change only
 * within 2 W intervals of them, and only where that interval's clean stretch was above 1.  A non-finite root entry reaches root
 * columns of the rows that read its row and nothing else: no need, no ticks.  No other clip changes.
 * GMR_EINVAL: negative counts, NULL arrays with work to do, window outside [0, 32], max_stretch outside [1, 64] (a NaN included),
 * fps not finite or not > 0, qpos_out == qpos, interp not 0 or 1.  GMR_EUNSUPPORTED: nq > 64 (a row does not fit one wavefront), a planar-base
 * model.  Zero work -- n_seq = 0; for apply also n_frames = 0 or n_out_frames = 0 -- returns GMR_OK without a launch.  With
 * n_frames = 0 and n_seq > 0 the plan still writes the clips' out_len, clip_stats and need_max (zeros).  Asynchronous on
 * in->stream; the handle's device is selected.
 * Layout (LP64): sizeof 120; offsets qpos 0, n_frames 8, seq_offsets 16, n_seq 24, window 28, fps 32, vmax 40, max_stretch 48,
 * stream 56, need 64, ticks 72, cum 80, out_len 88, clip_stats 96, need_max 104, reserved 112.  */
typedef struct gmr_retime_plan_input {
  const double  *qpos;            /* device [n_frames][nq] f64 */
  int64_t        n_frames;
  const int64_t *seq_offsets;     /* DEVICE [n_seq+1] */
  int32_t        n_seq, window;
  double         fps;
  const double  *vmax;            /* device [nq-7] f64 */
  double         max_stretch;
  void          *stream;          /* the call's stream */
  double        *need;            /* device [n_frames] f64 */
  int64_t       *ticks;           /* device [n_frames] i64 */
  int64_t       *cum;             /* device [n_frames] i64 */
  int64_t       *out_len;         /* device [n_seq] i64 */
  int64_t       *clip_stats;      /* device [n_seq][4] i64 */
  double        *need_max;        /* device [n_seq] f64 */
  int64_t        reserved;        /* 0 */
} gmr_retime_plan_input;
int gmr_motion_retime_plan(gmr_model *m, const gmr_retime_plan_input *in);

#define GMR_RETIME_INTERP_LINEAR 0
#define GMR_RETIME_INTERP_CUBIC 1
/* The second entry of the pair: the contract is above gmr_retime_plan_input.
 * Layout (LP64): sizeof 88; offsets qpos 0, n_frames 8, seq_offsets 16, ticks 24, cum 32, out_offsets 40, n_seq 48, interp 52,
 * n_out_frames 56, stream 64, qpos_out 72, src_time 80.  */
typedef struct gmr_retime_apply_input {
  const double  *qpos;            /* device [n_frames][nq] f64 */
  int64_t        n_frames;
  const int64_t *seq_offsets;     /* DEVICE [n_seq+1] */
  const int64_t *ticks;           /* device [n_frames] i64 */
  const int64_t *cum;             /* device [n_frames] i64 */
  const int64_t *out_offsets;     /* DEVICE [n_seq+1] */
  int32_t        n_seq, interp;   /* interp: GMR_RETIME_INTERP_LINEAR (0, the field's value when it was reserved) or _CUBIC */
  int64_t        n_out_frames;
  void          *stream;          /* the call's stream */
  double        *qpos_out;        /* device [n_out_frames][nq] f64, not qpos */
  double        *src_time;        /* device [n_out_frames] f64 */
} gmr_retime_apply_input;
int gmr_motion_retime_apply(gmr_model *m, const gmr_retime_apply_input *in);

/* Retiming to joint TORQUE limits: the plan of gmr_motion_retime_plan with the need taken from joint torques, for a clip that asks a
 * hinge for more torque than its actuator has.  Played slower by a locally constant factor s, a clip's velocities scale by 1/s and
 * its accelerations by 1/s^2, so a hinge's torque is tau(s) = g + (tau - g) / s^2, g the gravity torque of the pose: what
 * gmr_motion_dynamics returns when it is given qvel = qacc = 0.  Two calls of gmr_motion_dynamics on the same clips -- one
 * differenced, one static -- give tau and tau_static, and from them per row and hinge the exact smallest s that brings the hinge
 * under its limit.  What this leaves out is the term q' s' / s^2 of a stretch that changes along the clip: the caller meets it by
 * iteration (plan, gmr_motion_retime_apply with interp = GMR_RETIME_INTERP_CUBIC, dynamics again), which is why this entry has a
 * planning margin.  The plan feeds gmr_motion_retime_apply unchanged.  The call is its struct, the stream included; it enqueues
 * three kernels on in->stream (four with align_end) and nothing else: no allocation, no copy, no synchronisation.  All arrays are
 * device arrays.
 *   tau, tau_static   f64 [n_frames][nh], nh = nq - 7, hinges in qpos order: the torques of the clips and of their poses at rest
 *   seq_offsets, n_seq, n_frames, window, max_stretch    as for gmr_motion_retime_plan (the same clamping rule)
 *   torque_limit      f64 [nh], N m per hinge, every entry > 0; +inf: no limit.  Trusted (the Python layer checks it)
 *   limit_scale       in (0, 1]: the plan is made against limit_scale * torque_limit (the planning margin)
 *   need_floor        f64 [n_frames] or NULL: meant to be the need of a gmr_motion_retime_plan of the same clips, so that one
 *                     warp meets both limits
 *   align_end         0 or 1
 * All arithmetic is float64 without floating-point contraction, in the order written.  Per row r and hinge j:
 *   L = limit_scale * torque_limit[j],  g = tau_static[r][j],  d = tau[r][j] - g
 *   head = d >= 0 ? L - g : L + g                          what the limit leaves to the dynamic part, on the side it pushes to
 *   e_rj = 0 when torque_limit[j] is +inf, otherwise head > 0 ? fabs(d) / head : 0
 *   Gravity alone at or over the limit (head <= 0) is not something a slower clip mends: it contributes no need and is counted
 * Row r is NON-FINITE when any entry of its tau or tau_static row is not fabs(x) < +inf.
 *   rho_r = sqrt(max_j e_rj)                               one square root per row; 0 for a model without hinges
 *   static_over[r] = the number of hinges with a finite limit and fabs(g) >= L; 0 in a non-finite row
 * Interval i lies between the rows i and i + 1 of its clip and is stored at row i:
 *   need_i = max(rho_i, rho_{i+1});  with need_floor, need_i = max(need_i, need_floor[i])
 *   the interval is NON-FINITE when either row is, or when the floor is not < +inf: then need_i = NaN (0x7ff8000000000000), it
 *   stretches as 1, and it is counted.  The last row of a clip gets need 0 and ticks 0.
 * From need on -- s, d, m, ticks, cum, out_len, clip_stats and need_max -- the contract is gmr_motion_retime_plan's, word for word,
 * and so are the kernels.
 * align_end = 1.  out_len rounds a clip's total up, so the last output row would hold the final pose a fraction of a frame after
 * the row before it: an abrupt stop, and torques to match.  For a clip of n >= 2 rows with total t:
 *   r = (1024 - t % 1024) % 1024,  k = min(n - 1, 64)
 *   interval n - 1 - k + l (l = 0 .. k-1) gains r / k + (l < r % k) ticks; cum of the last k rows, out_len (= t' / 1024 + 1) and
 *   clip_stats[3] follow
 * The total is then a whole number of frames and the last output row is the final pose at its planned time.  No interval gains
 * more than 16 ticks once a clip has 65 rows; a clip of 2 rows rounds its one interval up to whole frames.  ticks may then exceed
 * 1024 max_stretch, by at most 1023.
 *   need, ticks, cum, out_len, clip_stats, need_max    as gmr_motion_retime_plan writes them
 *   static_over       i32 [n_frames], or NULL;  rows outside every clip are not written
 * GMR_EINVAL: negative counts, NULL arrays with work to do, window outside [0, 32], max_stretch outside [1, 64], limit_scale
 * outside (0, 1] (a NaN included), align_end not 0 or 1.  GMR_EUNSUPPORTED: nq > 64, a planar-base model.  n_seq = 0 returns
 * GMR_OK without a launch; with n_frames = 0 and n_seq > 0 the clips' out_len, clip_stats and need_max are written (zeros).
 * Asynchronous on in->stream; the handle's device is selected.
 * Layout (LP64): sizeof 144; offsets tau 0, tau_static 8, n_frames 16, seq_offsets 24, n_seq 32, window 36, torque_limit 40,
 * limit_scale 48, max_stretch 56, need_floor 64, align_end 72, reserved 76, stream 80, need 88, ticks 96, cum 104, out_len 112,
 * clip_stats 120, need_max 128, static_over 136.  */
typedef struct gmr_retime_torque_input {
  const double  *tau;             /* device [n_frames][nq-7] f64 */
  const double  *tau_static;      /* device [n_frames][nq-7] f64 */
  int64_t        n_frames;
  const int64_t *seq_offsets;     /* DEVICE [n_seq+1] */
  int32_t        n_seq, window;
  const double  *torque_limit;    /* device [nq-7] f64 */
  double         limit_scale;
  double         max_stretch;
  const double  *need_floor;      /* device [n_frames] f64, or NULL */
  int32_t        align_end, reserved;
  void          *stream;          /* the call's stream */
  double        *need;            /* device [n_frames] f64 */
  int64_t       *ticks;           /* device [n_frames] i64 */
  int64_t       *cum;             /* device [n_frames] i64 */
  int64_t       *out_len;         /* device [n_seq] i64 */
  int64_t       *clip_stats;      /* device [n_seq][4] i64 */
  double        *need_max;        /* device [n_seq] f64 */
  int32_t       *static_over;     /* device [n_frames] i32, or NULL */
} gmr_retime_torque_input;
int gmr_motion_retime_plan_torque(gmr_model *m, const gmr_retime_torque_input *in);

/* The per-clip quality report: what the reference's users gather by hand -- error1() / error2() per frame
 * (motion_retarget.py:188-200), per-task position errors, joints at their limits (mink.check_limits), the curated hard-motion
 * lists -- reduced on the device.  qpos and key-points are read once; the outputs are a few hundred bytes per clip.
 * Clip s holds the frames [seq_offsets[s], seq_offsets[s+1]).  Outputs are device arrays with n_seq rows, any may be NULL:
 *   err_max_out, err_sum_out [n_seq][2] f64        max / sum over the clip's frames of gmr_evaluate's err_out (0 for an unused table)
 *   task_pos_max_out, task_pos_sum_out [n_seq][nt] world distance |x_target - x_body| in metres of every task, target after
 *                                                  preparation; nt = ntask[0] + ntask[1], rows as in gmr_evaluate's task_err_out
 *                                                  (rows of an unused table are 0)
 *   task_rot_max_out, task_rot_sum_out [n_seq][nt] geodesic angle |w| in rad of the same task
 *   near_lo_out, near_hi_out [n_seq][nh] i32       frames with theta_j - lo_j <= limit_eps / hi_j - theta_j <= limit_eps, nh = nq - 7
 *                                                  hinges in qpos order; 0 for an unlimited hinge
 *   dof_step_max_out [n_seq][nh] f64               max |theta_j(t+1) - theta_j(t)| over consecutive frames of the clip
 *   root_step_max_out, root_turn_max_out [n_seq]   max root displacement (m) and max sign-blind geodesic angle (rad) between the
 *                                                  root orientations of consecutive frames; a planar base: xy distance and the
 *                                                  wrapped difference of the headings 2 atan2(qz, qw)
 *   solves_max_out [n_seq] i32, solves_sum_out [n_seq] i64   max / sum over the clip's frames of the solve counts in the optional
 *                                                  `iters` input (gmr_ik_solve's iters_out), bits 30 and 31 of every entry -- its
 *                                                  flags -- masked off (& 0x3FFFFFFF); a non-finite frame (below) is left out;
 *                                                  both outputs stay untouched when `iters` is NULL
 *   nonfinite_frames_out [n_seq] i32               frames whose qpos or consumed key-points hold a non-finite value; such a frame
 *                                                  enters no other statistic, and neither do the steps into and out of it
 * A clip without frames reports 0 everywhere; steps never cross clips.  The work unit is a segment of at most segment_frames
 * consecutive frames of one clip, one wavefront each; a second kernel folds a clip's segments in order, without floating-point
 * atomics: a report is bit-reproducible for a given segment_frames, and its maxima and counts do not depend on it.
 * The error fields need the key-points (GMR_EINVAL without them); seq_offsets follow gmr_motion_input's rules; a negative
 * segment_frames is GMR_EINVAL.  params NULL = the defaults.  Asynchronous on `stream`; the handle's device is selected.
 *   gmr_clip_report        one model
 *   gmr_group_clip_report  inputs host [group size]: member i's arguments (n_seq = 0: no work), all members' segments in one grid */
#define GMR_CLIP_REPORT_SEGMENT 32        /* frames per wavefront when segment_frames = 0 */
#define GMR_CLIP_REPORT_LIMIT_EPS 1e-3    /* rad: limit_eps when params is NULL */
typedef struct gmr_clip_report_input {
  const double *qpos;          /* device [n_frames][nq] f64 */
  int64_t n_frames;
  const void *human_pos, *human_quat;  /* device [n_frames][n_cols][3] / [4] wxyz, or both NULL (no error fields) */
  int32_t in_dtype, n_cols;    /* GMR_DTYPE_*, as in gmr_evaluate */
  const int32_t *slot_col;     /* host [nslot] */
  const int64_t *seq_offsets;  /* host [n_seq+1], 0 .. n_frames, non-decreasing (empty clips ok) */
  int32_t n_seq, reserved;
  const double *height_scale;  /* device [n_seq] f64 or NULL: per-clip factor on the human scale table */
  const int32_t *iters;        /* device [n_frames] i32 or NULL: gmr_ik_solve's iters_out (solves per frame, flag bits 30 / 31) */
  double *err_max_out, *err_sum_out;
  double *task_pos_max_out, *task_pos_sum_out, *task_rot_max_out, *task_rot_sum_out;
  int32_t *near_lo_out, *near_hi_out;
  double *dof_step_max_out, *root_step_max_out, *root_turn_max_out;
  int32_t *solves_max_out;
  int64_t *solves_sum_out;
  int32_t *nonfinite_frames_out;
} gmr_clip_report_input;
typedef struct gmr_clip_report_params {
  double limit_eps;            /* rad, >= 0 */
  int32_t segment_frames;      /* 0 = GMR_CLIP_REPORT_SEGMENT */
  int32_t offset_to_ground;    /* as gmr_ik_params.offset_to_ground */
} gmr_clip_report_params;
int gmr_clip_report(gmr_model *m, const gmr_clip_report_input *in, const gmr_clip_report_params *prm, void *stream);
int gmr_group_clip_report(gmr_group *g, const gmr_clip_report_input *inputs, const gmr_clip_report_params *prm, void *stream);

/* Single-sequence sessions ("teleop"): one frame per call, warm start carried in the session -- the semantics of calling
 * GeneralMotionRetargeting.retarget once per captured frame (motion_retarget.py:139-185).  Inputs and outputs are HOST
 * pointers: the session owns pinned, device-visible staging that the kernel reads and writes directly (no copy engines on
 * the path), one launch per frame on the session's own stream; gmr_session_step returns when qpos_out is filled.
 *   slot_col/in_dtype/n_cols/params as in gmr_ik_solve (params->offset_to_ground is overridden per step)
 *   human_pos host [n_cols][3], human_quat host [n_cols][4] wxyz, qpos_out host [nq] f64, solves_out host int32 or NULL
 *   gmr_session_reset: qpos host [nq] or NULL (= the model's qpos0, a fresh mink.Configuration)
 *   gmr_session_state: copies the current configuration to host [nq]
 * A session borrows its model: destroy sessions before the model.  Errors are reported on the model (gmr_last_error).     */
typedef struct gmr_session gmr_session;
gmr_session *gmr_session_create(gmr_model *m, int in_dtype, int n_cols, const int32_t *slot_col, const gmr_ik_params *params);
void gmr_session_destroy(gmr_session *s);
int gmr_session_reset(gmr_session *s, const double *qpos);
int gmr_session_step(gmr_session *s, const void *human_pos, const void *human_quat, int offset_to_ground, double *qpos_out,
                     int32_t *solves_out);
int gmr_session_state(gmr_session *s, double *qpos_out);
/* Persistent mode (idle_ms > 0): frames are handed to ONE resident wavefront through a pinned mailbox instead of a launch and a
 * stream synchronisation each -- the latency of a step drops from ~49 us to the wavefront's own solve time plus two PCIe hops.
 * The wavefront leaves by itself after idle_ms without a frame (and is relaunched by the next step), on reset / state / destroy,
 * and every wait inside it is bounded.  While it is resident, device-wide synchronisation (hipDeviceSynchronize, hipFree) waits
 * for it to idle out, which is why the mode is opt-in.  idle_ms = 0 returns to one launch per frame.  Results are identical. */
int gmr_session_set_persistent(gmr_session *s, int idle_ms);

/* Evaluate, per frame, the stage errors |concat_t Log(T_body^-1 T_target)| of both tables and/or the MuJoCo-convention FK.
 *   qpos device [n][nq] f64;  human_pos/human_quat/in_dtype/n_cols/slot_col as in gmr_ik_solve (needed only with err_out)
 *   height_scale device [n] f64 or NULL: per-frame factor on the human scale table (gmr_work_item.height_scale of the clip)
 *   err_out device [n][2] f64 or NULL;  xpos_out device [n][nbody][3] f64 or NULL;  xquat_out device [n][nbody][4] wxyz or NULL
 *   task_err_out device [n][ntask[0]+ntask[1]][6] f64 or NULL: FrameTask.compute_error of every task of table 1 then table 2
 *              (rows of an unused table are left untouched), Log(T_body^-1 T_target) as [v; w]
 * Non-finite input: a non-finite coordinate of qpos makes non-finite exactly the outputs of its own frame that are arithmetic
 * functions of it (the poses at and below its joint, the errors of the tasks on those bodies, the stage errors), and changes no
 * other output.  The root quaternion is normalised by a refined reciprocal square root of |q|^2: an infinite component makes all
 * four components of the root's xquat row NaN (0 x inf), not only itself. */
int gmr_evaluate(gmr_model *m, const double *qpos, int64_t n_frames, const void *human_pos, const void *human_quat, int in_dtype,
                 int n_cols, const int32_t *slot_col, int offset_to_ground, const double *height_scale, double *err_out,
                 double *task_err_out, double *xpos_out, double *xquat_out, void *stream);

/* Batched FK in the KinematicsModel convention (float32, xyzw).
 *   root_pos device [n][3], root_rot_xyzw device [n][4], dof device [n][nq-7]
 *   body_pos_out device [n][nbody][3]; body_rot_out device [n][nbody][4] or NULL
 * Non-finite input: a non-finite input coordinate makes non-finite exactly the outputs that are arithmetic functions of it, and
 * changes no other output: a root position coordinate reaches that coordinate of every body of its frame, a root quaternion
 * component every body but the root's position (and every rotation), a hinge angle the rotation of its body and the poses of the
 * bodies below it.  The same holds for gmr_fk_shape, gmr_dof_to_rot and gmr_local_rot_to_global; gmr_rot_to_dof keeps the
 * reference's selects: a quaternion whose |xyz| is not above 1e-5 -- a NaN in xyz included -- gives the angle 0, and the clamp to
 * the joint's range makes an infinite component a limit or 0.   */
int gmr_fk(gmr_model *m, const float *root_pos, const float *root_rot_xyzw, const float *dof, int64_t n_frames,
           float *body_pos_out, float *body_rot_out, void *stream);

/* The same with KinematicsModel.forward_kinematics' `fitted_shape`: every body's local translation is multiplied, in float32, by
 * its row of fitted_shape before the chain.
 *   fitted_shape device [nbody] (shape_width 1) or [nbody][3] (shape_width 3) float32, or NULL (= gmr_fk)
 * The scaled body table is the call's own (stream-ordered scratch): concurrent calls with different shapes do not interfere. */
int gmr_fk_shape(gmr_model *m, const float *root_pos, const float *root_rot_xyzw, const float *dof, const float *fitted_shape,
                 int shape_width, int64_t n_frames, float *body_pos_out, float *body_rot_out, void *stream);

/* The other KinematicsModel operators (float32, xyzw; hinge-or-fixed bodies as everywhere in this library; asynchronous on `stream`):
 *   gmr_dof_to_rot           dof device [n][nq-7]             -> joint_rot_out device [n][nbody-1][4]: the hinge quaternion of body
 *                            j+1's angle in row j, the identity for bodies without a hinge
 *   gmr_rot_to_dof           joint_rot device [n][nbody-1][4] -> dof_out device [n][nq-7]: angle about the joint axis of each hinge's
 *                            row (w made non-negative, 2 atan2(|xyz|, w), 0 below |xyz| = 1e-5, sign from the axis), clamped to the
 *                            joint's range
 *   gmr_local_rot_to_global  local_rot device [n][nbody][4]   -> global_rot_out device [n][nbody][4]: row 0 copied, every other row
 *                            global[parent] (x) local in the reference's operation order (results equal a sequential float32
 *                            evaluation bit for bit); the two arrays must not alias                                         */
int gmr_dof_to_rot(gmr_model *m, const float *dof, int64_t n_frames, float *joint_rot_out, void *stream);
int gmr_rot_to_dof(gmr_model *m, const float *joint_rot, int64_t n_frames, float *dof_out, void *stream);
int gmr_local_rot_to_global(gmr_model *m, const float *local_rot, int64_t n_frames, float *global_rot_out, void *stream);

/* Lowest body z per clip: min over frames [seq_offsets[s], seq_offsets[s+1]) and bodies of FK z.
 *   seq_offsets host [n_seq+1]; min_z_out device [n_seq] float32
 * low_s is the minimum of the clip's body heights when all of them are ordered.  It is NaN when any of them is NaN (torch.min's
 * rule, and the reference script's).  +-inf take part in the minimum as values.  A non-finite input coordinate changes the
 * minimum of its own clip only.                    */
int gmr_fk_min_height(gmr_model *m, const float *root_pos, const float *root_rot_xyzw, const float *dof,
                      const int64_t *seq_offsets, int n_seq, float *min_z_out, void *stream);

/* SMPL-X key-points (stateless): axis-angle joint rotations + joint positions -> global orientations (wxyz) and positions,
 * optionally resampled to n_frames_out frames at times linspace(0, n_frames-1, n_frames_out).
 *   parents host [n_joints] (parents[0] = -1, parents[j] < j);  joints_stride: joints per frame in `joints` (>= n_joints)
 *   global_orient device [n_frames][3], full_pose device [n_frames][n_joints][3], joints device [n_frames][joints_stride][3]
 *   pos_out device [n_frames_out][n_joints][3], quat_out device [n_frames_out][n_joints][4]                                */
int gmr_smplx_keypoints(const int32_t *parents, int n_joints, int joints_stride, const double *global_orient, const double *full_pose,
                        const double *joints, int64_t n_frames, int64_t n_frames_out, int resample, double *pos_out, double *quat_out,
                        void *stream);

/* The same with a column selection: out_cols host [n_out] names the joints to emit, column c of the outputs = joint out_cols[c]
 * (each at most once); their ancestors are chained internally, joints that are neither emitted nor an ancestor of an emitted one are
 * not read.  With the 14 joints an smplx_to_*.json config consumes, gmr_ik_solve reads a dense [n_frames_out][14][7] instead of
 * picking 14 of 55 columns.  out_cols == NULL: all joints (n_out ignored).
 *   pos_out device [n_frames_out][n_out][3], quat_out device [n_frames_out][n_out][4]                                        */
int gmr_smplx_keypoints_cols(const int32_t *parents, int n_joints, int joints_stride, const double *global_orient, const double *full_pose,
                             const double *joints, int64_t n_frames, int64_t n_frames_out, int resample, const int32_t *out_cols, int n_out,
                             double *pos_out, double *quat_out, void *stream);

/* The same for input arrays of either element type: in_dtype GMR_DTYPE_F32 (what a body model emits: the arrays go in as they are,
 * each element promoted to float64 on load -- exactly what the reference's scipy / numpy calls do with float32 input -- at half the
 * bytes) or GMR_DTYPE_F64.  global_orient, full_pose, joints: device arrays of that type, shapes as above.                        */
int gmr_smplx_keypoints_in(const int32_t *parents, int n_joints, int joints_stride, const void *global_orient, const void *full_pose,
                           const void *joints, int in_dtype, int64_t n_frames, int64_t n_frames_out, int resample, const int32_t *out_cols,
                           int n_out, double *pos_out, double *quat_out, void *stream);

/* The SMPL-X body model's joints from AMASS parameters, for every clip of a batch in one launch: what load_smplx_file
 * (general_motion_retargeting/utils/smpl.py:12-41) takes from the `smplx` package for the first 55 joints, without the vertices.
 * Per clip the rest joints J = j_template + j_dirs betas are formed on the device, then per frame
 *   full_pose      row 0 root_orient, rows 1-21 pose_body, rows 22-24 zero, rows 25-54 hand_mean (the model's mean hand pose)
 *   global_orient  root_orient
 *   joints         R_0 = exp(root_orient), p_0 = J_0; R_i = R_parent exp(full_pose_i), p_i = p_parent + R_parent (J_i - J_parent); + trans
 * with the exponential map and the products of gmr_smplx_keypoints_in, so the orientations that call derives from full_pose are
 * the rotations these positions were built with.  Clip c's frames are rows sum(n_frames of the clips before it) ... of the outputs.
 *   parents host [n_joints], n_joints = 55 (GMR_EUNSUPPORTED otherwise)
 *   clips host [n_clips]; root_orient / pose_body / trans device [n_frames][3 / 63 / 3] of element type in_dtype[0 / 1 / 2];
 *     j_template device [55][3], j_dirs device [55][3][dirs_stride], hand_mean device [90] (float64); betas HOST [n_betas <= dirs_stride]
 *   out_cols / n_out as in gmr_smplx_keypoints_cols: only the named joints and their ancestors are evaluated AND WRITTEN (the rows
 *     that call reads with the same selection); the other joints' entries of full_pose / joints are left as they are
 *   global_orient device [N][3], full_pose device [N][55][3], joints device [N][55][3] (float64)
 *   rest_out device [n_clips][55][3] or NULL: the clips' rest joints
 * Asynchronous on `stream`; the device of the outputs is selected; scratch comes from the library's own pool.               */
typedef struct gmr_smplx_body_clip {
  const void *root_orient, *pose_body, *trans;
  const double *j_template, *j_dirs, *hand_mean;
  const double *betas;
  int64_t n_frames;
  int32_t in_dtype[3];
  int32_t n_betas, dirs_stride, reserved;
} gmr_smplx_body_clip;
int gmr_smplx_body(const int32_t *parents, int n_joints, const gmr_smplx_body_clip *clips, int n_clips, const int32_t *out_cols, int n_out,
                   double *global_orient, double *full_pose, double *joints, double *rest_out, void *stream);

/* Host-side parse of a BVH file's HIERARCHY section and MOTION header (stateless, no device involved; grammar and the
 * reference semantics it keeps are documented in gmr_amd/csrc/bvh_text.h).  Replaces the hierarchy loop of read_bvh
 * (general_motion_retargeting/utils/lafan_vendor/extract.py:60-139).
 *   text/len        the file (or at least its header)
 *   names_out       host char[names_cap]: joint names, NUL-separated, in hierarchy order
 *   parents_out     host int32[max_joints] (-1 for the root); offsets_out host double[max_joints][3]
 *   channels_out    host int32[max_joints]: channel count of every joint
 *   order_out       host int32[3]: axes (0=x,1=y,2=z), in listed order, of the first joint whose rotation slice -- channels 0-2 of a
 *                   3-channel joint, 3-5 of any other -- is all rotations (a positions-only root of the 9-channel layout is skipped)
 *   n_frames_out, frame_time_out: the MOTION header; motion_offset_out: byte offset of the first motion row in text
 * Returns the number of joints, -1 on a malformed file, -2 if max_joints / names_cap are too small.                      */
int gmr_bvh_parse_header(const char *text, size_t len, int max_joints, char *names_out, size_t names_cap, int32_t *parents_out,
                         double *offsets_out, int32_t *channels_out, int32_t *order_out, int64_t *n_frames_out, double *frame_time_out,
                         size_t *motion_offset_out);

/* Host-side text parse of a BVH MOTION block (stateless, no device involved): the first max_lines non-empty lines of
 * text[0..len) are read as whitespace-separated decimal numbers into out (host, capacity max_out doubles), correctly
 * rounded like Python's float().  *n_lines = lines read, *n_cols = numbers on the first line.  Returns the count of numbers
 * written, or -1 on a malformed token, a line whose length differs from the first, or an overflow of max_out.            */
int64_t gmr_bvh_parse_motion(const char *text, size_t len, int64_t max_lines, double *out, int64_t max_out, int64_t *n_lines,
                             int64_t *n_cols);

/* The same parse on the device, for a batch of files whose text is already in device memory (one H2D copy of the files as they
 * are): identical values, bit for bit, for every token on the exact fast path (at most 19 significant digits, mantissa < 2^53, power
 * of ten within 10^+-22: one correctly rounded multiply / divide, what float() returns); every other token is REPORTED, not guessed:
 * the caller parses those with strtod (gmr_bvh_parse_motion's slow path) and patches rows_out.  Replaces the same reference lines
 * (general_motion_retargeting/utils/lafan_vendor/extract.py:140-156).
 *   text        device [text_bytes]   the files' bytes; seg_begin/seg_end host [n_files]: each file's MOTION block in it
 *   n_lines     host [n_files]  rows to read per file (the header's Frames:);  n_cols: numbers per row (one skeleton per batch)
 *   row_begin   host [n_files]  first row of each file in rows_out;  rows_out device [sum(n_lines)][n_cols] float64
 *   status_out  host [n_files]  0 = ok; bit 0: some row does not hold n_cols numbers, bit 1: fewer than n_lines rows -- parse that
 *               file with gmr_bvh_parse_motion, which reports what is wrong with it
 *   n_tokens_out host [n_files] or NULL: numbers found in the whole block
 *   slow_out    host [max_slow][3]  (file, index of the number in its file, byte offset in text) of the tokens off the fast path;
 *               *n_slow = how many there were (more than max_slow: treat the files as status != 0)
 * Runs on `stream` and synchronises it before returning.                                                                   */
int gmr_bvh_parse_motion_device(const char *text, int64_t text_bytes, int n_files, const int64_t *seg_begin, const int64_t *seg_end,
                                const int64_t *n_lines, int64_t n_cols, const int64_t *row_begin, double *rows_out, int32_t *status_out,
                                int64_t *n_tokens_out, int64_t *slow_out, int64_t max_slow, int64_t *n_slow, void *stream);

/* BVH skeleton FK (stateless).  Joints in hierarchy order (parents[0] = -1, parents[j] < j), one Euler triple per joint.
 *   parents, euler_order[3] (0=x,1=y,2=z, the order the channels are listed), extra_*_src[n_extra]: host
 *   local_pos  device [n_frames][n_joints][3]  local translations (file units)
 *   euler_rad  device [n_frames][n_joints][3]  channel angles in radians
 *   pos_out    device [n_frames][n_joints+n_extra][3]  = scale * (global position rotated to Z-up)
 *   quat_out   device [n_frames][n_joints+n_extra][4]  wxyz, rotated to Z-up
 * Extra entry k takes the position of joint extra_pos_src[k] and the orientation of joint extra_rot_src[k].        */
int gmr_bvh_fk(const int32_t *parents, int n_joints, const int32_t *euler_order, const int32_t *extra_pos_src,
               const int32_t *extra_rot_src, int n_extra, const double *local_pos, const double *euler_rad, int64_t n_frames,
               double scale, double *pos_out, double *quat_out, void *stream);

/* The same fed with the file's own motion rows, as gmr_bvh_parse_motion wrote them (degrees, file units): the slicing of a row into
 * root translation / per-joint channels (general_motion_retargeting/utils/lafan_vendor/extract.py:140-156) and the degrees -> radians
 * step of load_lafan1_file (utils/lafan1.py:13) happen in the kernel, so nothing is reshaped or copied on the host.
 *   channels   3: rows = 3 root position values + 3 angles per joint;  6: (position, angles) per joint;
 *              9: 3 root position values + (position, angles, scale) per non-root joint, local position = offset + position * scale,
 *                 zero root rotation
 *   offsets    device [n_joints][3]  the joints' OFFSET lines (local positions where the rows carry none)
 *   rows       device [n_frames][n_cols]
 *   out_cols   host [n_out] or NULL: entries (joint j, or n_joints + k for extra k) to emit, column c = entry out_cols[c];
 *              NULL = all n_joints + n_extra
 *   pos_out    device [n_frames][n_out][3], quat_out device [n_frames][n_out][4]                                                  */
int gmr_bvh_fk_rows(const int32_t *parents, int n_joints, const int32_t *euler_order, const int32_t *extra_pos_src,
                    const int32_t *extra_rot_src, int n_extra, int channels, const double *offsets, const double *rows, int64_t n_cols,
                    int64_t n_frames, double scale, const int32_t *out_cols, int n_out, double *pos_out, double *quat_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GMR_AMD_H */
