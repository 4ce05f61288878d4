/* yolo_fastest_hip.h -- C ABI of libyolo_fastest_hip.so (MI355X / gfx950).
 *
 * The reference (JunFenngZhi/YOLO-Fastest-and-Embedded-deployment) has no FFI for its inference
 * path: the boundary is its Python surface.  Each entry point below replaces the body of one
 * Python-level call of the reference; the Python host code in
 * yolo-fastest-and-embedded-deployment_amd/ keeps the reference's names and argument meaning and
 * binds these symbols with ctypes (INTEGRATION.md shows the stub).
 *
 *   reference interface (file:line under the reference repo)            entry point
 *   ------------------------------------------------------------------  -------------------
 *   YoloFastest(io_params).to(dev).eval() + load_state_dict(torch.load) yf_create
 *       src/model_training/model/yolo_fastest.py:70-148, src/detect.py:89-91
 *   model(img) -> (head_large, head_small)                               yf_forward
 *       src/model_training/model/yolo_fastest.py:150-218, src/detect.py:152
 *   YOLO_post_process.decode_box + class bucketing + sort + NMS          yf_decode_nms
 *       src/detect.py:41-84, :157-169   (+ __adjust_coord :131-139 when origin_* given)
 *   YOLO_post_process.non_maxium_supression(sorted_list)                 yf_nms_sorted
 *       src/detect.py:69-84
 *   Detect_YOLO.batch_detect's timed region (model + post-process)       yf_detect
 *       src/detect.py:151-171
 *   Detect_YOLO.__pre_process's arithmetic ((u8-128)/255, 2x2 area mean) yf_preprocess_u8
 *       src/detect.py:107-129
 *
 * Conventions: plain pointers and sizes only.  Every pointer named d_* is DEVICE memory owned by the
 * caller (a torch tensor's data_ptr()); `stream` is a hipStream_t passed as void*.  All launches are
 * stream-ordered and asynchronous; nothing here synchronises the device except yf_create /
 * yf_destroy.  Return value: 0 = ok, negative = error (see YF_E_*); yf_last_error_string() gives
 * the message of the calling thread's last failure.  A handle is bound to one device and is not
 * thread-safe (one handle per device per thread, as the reference's caller is single-threaded).
 */
#ifndef YOLO_FASTEST_HIP_H
#define YOLO_FASTEST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct yf_engine *yf_handle;

enum {
    YF_OK = 0,
    YF_E_INVALID = -1,   /* bad argument (shape not multiple of 32, N > max_batch, null pointer, ...) */
    YF_E_BLOB = -2,      /* packed-weights blob does not describe YoloFastest (strict layout check)  */
    YF_E_HIP = -3,       /* a HIP runtime call failed                                                */
    YF_E_WORKSPACE = -4, /* caller's workspace too small                                             */
    YF_E_NOPROBE = -5    /* yf_forward_probe: tensor of that name never exists in device memory      */
};

/* ABI version of this header; yf_abi_version() must return the same number. */
#define YF_ABI_VERSION 1
int yf_abi_version(void);

/* Thread-local message of the last failing call ("" if none). */
const char *yf_last_error_string(void);

/* Build an engine for net-input size H x W (rows x cols, multiples of 32) from a packed-weights blob
 * (host memory; format: yolo-fastest-and-embedded-deployment_amd/packer.py -- BN-folded fp32, NHWC-friendly
 * layouts, self-describing layer table that is checked strictly against the YoloFastest graph).
 * The engine owns a device copy of the weights and nothing else.
 * The blob's header carries the io_params the reference's constructor reads (src/model_training/model/yolo_fastest.py:72-78):
 * input_channel (1 = gray, 3 = cv2's BGR frames; conv0's Cin, :78), num_anchors and num_cls (num_out = num_anchors * (5 + num_cls)
 * channels per head, :76, :138, :148).  Below, C_in = input_channel, A = num_anchors (<= 8), C = num_cls, num_out = A * (5 + C);
 * the shipped checkpoints are C_in = 1, A = 3, C = 3, num_out = 24.  yf_io_params() reads them back. */
int yf_create(const void *packed_weights, size_t nbytes, int H, int W, int max_batch, int device, yf_handle *out);
/* dtype 0 = fp32 (yf_create); 1 = BASELINE configs[2]: activations stored fp16 in HBM, the pointwise GEMMs on
 * v_mfma_f32_16x16x16_f16 with fp16 weights, fp32 accumulation everywhere; depthwise / small-channel kernels compute in fp32
 * on fp16 storage.  Input x and the two head tensors stay fp32.  (model.half() selects it from Python.) */
/* dtype 2 = fp32 storage everywhere (HBM and LDS: the residual trunk is never rounded), the pointwise GEMMs on the fp16 matrix
 * pipe with SPLIT operands: every MFMA operand a is carried as two fp16 halves hi = rne(a), lo = rne(a - hi) (22 bits) and a k-group
 * issues w_lo*a_hi + w_hi*a_lo + w_hi*a_hi into the fp32 accumulator.  As accurate as dtype 0 (same distance from the graph in fp64);
 * the accuracy answer to BASELINE configs[2]'s "2e-2 on logits", which single fp16 operands cannot meet (weights alone: 4.5e-2). */
int yf_create_ex(const void *packed_weights, size_t nbytes, int H, int W, int max_batch, int device, int dtype, yf_handle *out);
/* The fp32 -> fp16 rounding (nearest even) the weight packer uses on the host. */
uint16_t yf_f32_to_f16_bits(float f);
int yf_destroy(yf_handle h);
int yf_io_params(yf_handle h, int *input_channel, int *num_anchors, int *num_cls, int *num_out);   /* any pointer may be NULL */

/* Bytes of device scratch yf_forward / yf_detect need for a batch of N frames. */
int yf_workspace_bytes(yf_handle h, int N, size_t *out);

/* model(x): d_x float32 [N,C_in,H,W] contiguous (NCHW like the reference's input), values (u8-128)/255.
 * d_head_large float32 [N,num_out,H/16,W/16], d_head_small float32 [N,num_out,H/32,W/32], NCHW like the reference. */
int yf_forward(yf_handle h, const float *d_x, int N, float *d_head_large, float *d_head_small,
               void *d_workspace, size_t workspace_bytes, void *stream);

/* Test hook: run the forward pass and copy the named intermediate activation (the output of the
 * reference module attribute `name`, e.g. "conv1_9", "res3_3"), converted to NCHW float32
 * [N,C,h,w], into d_dst.  Returns YF_E_NOPROBE for tensors that a fused kernel keeps on chip. */
int yf_forward_probe(yf_handle h, const float *d_x, int N, const char *name, float *d_dst, size_t dst_bytes,
                     void *d_workspace, size_t workspace_bytes, void *stream);

/* Post-process of N frames (the reference handles batch element 0 only, detect.py:46; frame f here is
 * exactly what the reference computes for pred[f:f+1]).
 *   anchors: HOST double[2][A][2] = io_params["anchors"][head][anchor][w,h] in net-input pixels (the first A of each group,
 *       detect.py:51,63-64).  Classes: argmax over the C raw class logits, first maximum wins (detect.py:59).
 *   conf_thres / nms_thres: strict '>' as in detect.py:58,79.
 *   origin_h/origin_w: if both > 0 and different from H/W, corners are rescaled and re-rounded as
 *       __adjust_coord does (detect.py:131-139); pass 0,0 to keep net-input coordinates.
 * Outputs (device), fixed capacity K_max per frame, survivors in the reference's order
 * (class-major; within a class conf descending, ties in decode order):
 *   d_boxes   int32 [N,K_max,4]  x1,y1,x2,y2
 *   d_scores  float [N,K_max,2]  conf, cls_score  (computed in fp64, stored fp32)
 *   d_cls     int32 [N,K_max]
 *   d_src     int32 [N,K_max]    flat index over (head, anchor, row, col) of the surviving cell
 *   d_counts  int32 [N]          survivors of frame f; if more than K_max survive the first K_max are
 *                                stored and the count is the TRUE number (caller detects overflow);
 *                                -2 = the reference would raise ZeroDivisionError (two zero-area boxes
 *                                compared, detect.py:39)
 */
int yf_decode_nms(yf_handle h, const float *d_head_large, const float *d_head_small, int N, double conf_thres,
                  double nms_thres, const double *anchors, int origin_h, int origin_w, int K_max, int32_t *d_boxes,
                  float *d_scores, int32_t *d_cls, int32_t *d_src, int32_t *d_counts, void *stream);

/* The same with ONE output: d_records int32 [N, 1 + 8 K_max], one row per frame =
 *   count | boxes x1,y1,x2,y2 (4 K_max) | conf, cls_score as float32 bit patterns (2 K_max) | cls (K_max) | src (K_max)
 * -- the record block the multi-GPU exchange sends (one all-gather of fixed-capacity records per step): the collective
 * takes the kernel's own output buffer, nothing is packed or copied on the way.  Entries beyond `count` are not written. */
int yf_decode_nms_packed(yf_handle h, const float *d_head_large, const float *d_head_small, int N, double conf_thres, double nms_thres,
                         const double *anchors, int origin_h, int origin_w, int K_max, int32_t *d_records, void *stream);

/* YOLO_post_process.non_maxium_supression (detect.py:69-84) on its own: d_boxes int32 [n,4] is ONE class's
 * list already sorted by conf descending.  d_suppressor int32 [n] receives -1 for a kept box, else the index
 * of the kept box that removed it (-2 in every entry: the reference's ZeroDivisionError). */
int yf_nms_sorted(yf_handle h, const int32_t *d_boxes, int n, double nms_thres, int32_t *d_suppressor, void *stream);

/* Validation-time decode and NMS (the reference's OTHER convention, used by validate.py for mAP):
 *   yf_val_decode_head = YOLOLossV3.forward(input, targets=None)   src/model_training/loss/yolo_loss.py:48-68, :98-141
 *       d_head float32 [N,num_out,fh,fw] -> rows m_off .. m_off+A*fh*fw of d_out float32 [N,M_total,5+C] = (cx,cy,w,h,conf,cls0..),
 *       anchors: HOST double[A][2] of this head; calling it once per head with m_off = 0 / A*fh*fw reproduces
 *       validate.py:38-42's torch.cat over heads.  (The reference's own decode branch repeats its grid 3 times, yolo_loss.py:110-111,
 *       and therefore only runs with 3 anchors; this one takes any A.)
 *   yf_val_nms = utils.general.non_max_suppression                 src/model_training/utils/general.py:87-143 (+ bbox_iou :29-52)
 *       d_pred float32 [N,M,5+C] (yf_val_nms: C = the engine's num_cls; yf_val_nms_ex: C = num_classes, the reference's argument);
 *       conf >= conf_thres, per-class greedy NMS, IoU with the +1 convention, keep iou < nms_thres;
 *       d_det float32 [N,K_max,7] = (x1,y1,x2,y2,obj_conf,class_conf,class_pred), class-ascending then conf-descending;
 *       d_counts int32 [N] = true number of detections (0 <=> the reference's None);
 *       M <= 8191 and num_classes < 2^18 (the fields of the 64-bit sort key), else YF_E_INVALID; equal confidences keep row order. */
int yf_val_decode_head(yf_handle h, const float *d_head, int N, int fh, int fw, const double *anchors, int M_total, int m_off,
                       float *d_out, void *stream);
int yf_val_nms(yf_handle h, const float *d_pred, int N, int M, double conf_thres, double nms_thres, int K_max, float *d_det,
               int32_t *d_counts, void *stream);
int yf_val_nms_ex(yf_handle h, const float *d_pred, int N, int M, int num_classes, double conf_thres, double nms_thres, int K_max,
                  float *d_det, int32_t *d_counts, void *stream);

/* Validation's matching of detections to ground truth for a whole batch: Validation.get_mAP's per-image loop
 *                                                                      src/model_training/validate.py:46-74 (+ bbox_iou, utils/general.py:29-52)
 *   d_det, d_counts: yf_val_nms_ex's output as it is (K_max the same); an image contributes min(max(count, 0), K_max) detections.
 *   d_targets float32 [N,T,6] = (x1, y1, x2, y2, class, marker) in net-input pixels (validate.py:112-122's recovered corners); only rows
 *       with marker > 1 exist (validate.py:47).  T = 0: every detection is a false positive.  T <= 65536.
 *   Per image, detections in slot order (class-ascending, then confidence-descending = validate.py:50's unique() loop over :56's): a
 *       detection is a true positive if a target not yet matched has class == class_pred (compared as floats) and IoU (fp32, +1
 *       convention, clamp(min=0) on both extents, / (a1 + a2 - inter + 1e-16f)) > (float)iou_thres; the one with the lowest index is taken
 *       and removed.  NaN behaves as in torch (max / min / clamp return it): a NaN IoU is not above the threshold.
 *   d_records int32 [cap,3]: one record per detection = (obj_conf as float32 bits, (int)class_pred, hit 0 / 1), appended in image, slot
 *       order from record *d_base on; a record whose index is >= cap is not written.  *d_next = *d_base + the number of this call's
 *       detections, written or not: pass it as the next call's d_base (two int64 slots used in turn; d_next == d_base is refused).
 *   `device` = HIP device index; stream-ordered, no allocation, no synchronisation, plain vector stores only.
 *   YF_E_INVALID before any launch: a null pointer, N < 1, K_max < 1, T < 0 or > 65536, cap < 0. */
int yf_val_match(int device, const float *d_det, const int32_t *d_counts, int N, int K_max, const float *d_targets, int T, double iou_thres,
                 const int64_t *d_base, int64_t *d_next, int32_t *d_records, int64_t cap, void *stream);

/* The same detections scored as yolov5 scores them (its val.py process_batch, v6.1 and later, where the second re-sort by IoU is commented
 * out), at num_thresholds IoU thresholds in one launch per batch.  Not in the reference; yf_val_match above is untouched.
 *   d_det, d_counts, d_targets, N, K_max, T as for yf_val_match (detections in slot order, a row is a target only with marker > 1), but
 *       T <= 512: an image's winner table int32 [num_thresholds][T] sits in LDS.
 *   iou_thresholds: HOST double[num_thresholds], 1 <= num_thresholds <= 16, each cast to float; every one finite, as a float too.
 *   IoU = yolov5's box_iou in fp32, no +1: iw = clamp0(min(d.x2, t.x2) - max(d.x1, t.x1)), ih likewise, inter = iw * ih,
 *       iou = inter / ((area_t + area_d) - inter + 1e-7f), area = (x2 - x1) * (y2 - y1); min, max and clamp return NaN as torch does.
 *   Best target b(k) of detection k: the target of class == class_pred (compared as floats) with the largest non-NaN IoU, the lowest index
 *       among equals; none if there is no such target.  It does not depend on the threshold.
 *   At threshold j, k is a candidate if iou(k, b(k)) >= (float)iou_thresholds[j]; among the candidates that share a target the lowest
 *       slot k wins, the others get no hit at j.  Bit j of a detection's hit mask is set iff it is the winner of its target at j.
 *       Where no detection has two same-class targets at equal IoU this is process_batch's result exactly; on such ties yolov5's own result
 *       depends on numpy's unstable default sort, and the lowest-index rule is this library's definition.
 *   d_records int32 [cap,4]: one record per detection = (obj_conf as float32 bits, class_conf as float32 bits, (int)class_pred, hit mask),
 *       in image, slot order; cursor (d_base, d_next), cap and the clipping of the counts exactly as for yf_val_match.
 *   The result does not depend on the order the hardware runs anything in.  Stream-ordered, no allocation, no synchronisation, plain
 *   vector stores and LDS atomics only.
 *   YF_E_INVALID before any launch: a null pointer, N < 1, K_max < 1, T < 0 or > 512, cap < 0, num_thresholds < 1 or > 16, a threshold
 *   that is NaN or infinite (as a double or once cast to float), d_next == d_base. */
int yf_val_match_iouv(int device, const float *d_det, const int32_t *d_counts, int N, int K_max, const float *d_targets, int T,
                      const double *iou_thresholds, int num_thresholds, const int64_t *d_base, int64_t *d_next, int32_t *d_records,
                      int64_t cap, void *stream);

/* yolov5's own NMS (v6.1 / v7.0 utils/general.py::non_max_suppression, with torchvision.ops.nms stated as its CPU kernel's loop) on the same
 * decoded rows, one launch per batch.  Not in the reference; yf_val_nms / yf_val_nms_ex above are untouched.  Neither yolov5 nor
 * torchvision was available where this was written: the rule below is the definition, and parity with a real torchvision build is
 * unpinned (as the OpenCV restatements' parity with a real OpenCV build is).  All arithmetic is fp32.  Per image, on d_pred float32
 * [N,M,5+C] rows (cx, cy, w, h, obj, cls_0 ..):
 *   Candidate rows: obj > (float)conf_thres -- strict, a NaN fails.  Corners x1 = cx - w/2, y1 = cy - h/2, x2 = cx + w/2, y2 = cy + h/2.
 *       Scores s_j = cls_j * obj (an fp32 product).  multi_label holds only if the argument is non-zero AND C > 1.
 *   Candidates, with multi_label: every (m, j) with s_j > conf_thres, candidate index m * C + j.  Without: one per row, j = the first index
 *       of the largest s_j, kept if s_j > conf_thres, candidate index m; a row with a NaN score is dropped (torch.max hands the NaN on).
 *   Ranking: by s descending, equal scores by the lowest candidate index -- this library's definition: torch's argsort is unstable
 *       there, so yolov5's own order among equal scores is whatever its sort leaves.  Only the first max_nms stay.
 *   Suppression: c = agnostic ? 0 : (float)j * 7680.0f; the suppression sees b = (x1 + c, y1 + c, x2 + c, y2 + c), each sum rounded to
 *       fp32 as yolov5's are, and area = (b.x2 - b.x1) * (b.y2 - b.y1).  Walk the candidates in rank order; one that is still live is
 *       kept, and every later live q dies iff inter / (area + area_q - inter) > (float)iou_thres, where
 *       inter = max(0, min(x2, q.x2) - max(x1, q.x1)) * max(0, min(y2, q.y2) - max(y1, q.y1)) and min(a, b) = (b < a) ? b : a,
 *       max(a, b) = (a < b) ? b : a (std::min / std::max: a NaN second operand is dropped, a NaN first one stays).  No epsilon, no +1:
 *       0 / 0 is NaN and suppresses nothing.  Stop after max_det keeps.
 *   d_det float32 [N,K_max,7]: the kept candidates in rank order (confidence-descending across classes, the order process_batch assumes)
 *       = (x1, y1, x2, y2 WITHOUT the offset, obj, cls_j as read, (float)j): yf_val_nms_ex's record layout, which yf_val_match_iouv and
 *       the fp32 product obj * cls_j (commutative: yolov5's conf bit for bit) consume unchanged.  d_counts int32 [N] = number kept, at
 *       most max_det.  Slots past the count, and kept candidates past K_max, are not written.  A corner that the arithmetic makes NaN
 *       (inf - inf) is a NaN; WHICH NaN (sign, payload) is the processor's choice and unspecified.  Values copied from d_pred keep their bits.
 *   d_work: yf_val_nms_v5_work_bytes(N, M, num_classes, multi_label) bytes of device scratch, 8-byte aligned (0 from the helper: its
 *       arguments are refused below).  With B = M * C (multi_label) or M candidates at most, padded to a power of two P >= 64, an image's
 *       table is P 8-byte sort keys (~score bits << 32 | candidate index: no limit on M besides M * C <= 2^31 - 1) and P liveness bytes.
 *       It sits in LDS when 9 P + YF_VAL_NMS_V5_LDS_STATIC <= YF_VAL_NMS_V5_LDS_BUDGET (P <= 16384), and d_work is then not touched;
 *       otherwise in the image's 9 P bytes of d_work.  The result is the same either way.
 *   Not built: the `classes` filter, `labels` autolabelling, `merge`, the wall-clock `time_limit` break, and val.py's rescale and clip of
 *       the boxes to the original image size.
 *   `device` = HIP device index; stream-ordered, no allocation, no synchronisation, plain vector stores only.
 *   YF_E_INVALID before any launch: a null pointer, N < 1, M < 1, num_classes < 1, M * num_classes > 2^31 - 1, conf_thres NaN or negative
 *   (the sort key needs positive score bits to be monotone), iou_thres NaN, max_det < 1, max_nms < 1, K_max < 1, work_bytes below the
 *   helper's value. */
#define YF_VAL_NMS_V5_LDS_BUDGET 163840  /* bytes of LDS one workgroup may use: MI355X has 160 KiB per CU, all of it open to one workgroup */
#define YF_VAL_NMS_V5_LDS_STATIC 256     /* of which reserved for the kernel's own counters */
int yf_val_nms_v5(int device, const float *d_pred, int N, int M, int num_classes, double conf_thres, double iou_thres,
                  int multi_label, int agnostic, int max_det, int max_nms, int K_max,
                  void *d_work, size_t work_bytes, float *d_det, int32_t *d_counts, void *stream);
size_t yf_val_nms_v5_work_bytes(int N, int M, int num_classes, int multi_label);

/* The loss end of the reference's training step (first slice; the layers' backward is not part of it):
 *   yf_train_loss = YOLOLossV3.forward(input, targets) for ONE head   src/model_training/loss/yolo_loss.py:48-97 (+ get_target :144-196)
 *                   and, if d_grad_head is not NULL, d(total loss)/d(input): what loss.backward() (train.py:131) leaves in input.grad.
 *   d_head float32 [N,A*(5+C),fh,fw]; anchors: HOST double[A][2] of this head (net-input pixels; yf_train_loss: A, C of the engine;
 *   yf_train_head_loss: 3, 3; yf_train_head_loss_ex: as given -- yolo_loss.py:28-33); d_targets float32 [N,T,6] =
 *   (x, y, w, h normalised to 0..1, class, marker >= 1; the first row with marker < 1 ends an image's list, yolo_loss.py:158);
 *   ignore_thres = config train_params.IOU_loss_thre.
 *   d_losses float32 [8] = total, x, y, w, h, conf, cls (the 7-tuple of yolo_loss.py:94-95) and, in [7], the number of targets the
 *   reference cannot index: the cell (int(x * fw), int(y * fh)) lies outside the feature map, or the class int(class) lies outside
 *   0 .. C-1 (yolo_loss.py:195).  The reference raises IndexError for those; here such a target is skipped whole (no mask, no box, no
 *   class, no ignore mark), counted, and the caller decides (validation.YOLOLossV3 raises IndexError).  One departure: a NEGATIVE
 *   column, row or class index wraps round in the reference (Python indexing); that is not reproduced, it is counted like the rest.
 *   d_work: yf_train_loss_workspace_bytes(N, fh, fw) bytes of device scratch, 8-byte aligned.  Its layout is fixed (the tests read
 *   the target planes back): double[16] -- [0..6] the sums of the x, y, w, h, conf-object, conf-no-object and class terms over the
 *   cells, [7] the number of positive cells, [8] the count reported in d_losses[7], the rest zero -- then, with E = N*A*fh*fw cells in
 *   d_head's (n, anchor, row, column) order, float32 [6 + C][E]: the planes mask, noobj_mask, tx, ty, tw, th, class 0 .. C-1 of
 *   get_target (yolo_loss.py:144-196); up to 64 bytes behind them are reserved and not written. */
int yf_train_loss_workspace_bytes(yf_handle h, int N, int fh, int fw, size_t *out);
int yf_train_loss(yf_handle h, const float *d_head, int N, int fh, int fw, const double *anchors, const float *d_targets, int T,
                  double ignore_thres, void *d_work, size_t work_bytes, float *d_losses, float *d_grad_head, void *stream);
/* The same without an engine: H x W = the net input (only the head's stride is taken from it), like the other yf_train_* entries. */
int yf_train_head_loss_workspace_bytes(int N, int fh, int fw, size_t *out);
int yf_train_head_loss(int device, int H, int W, const float *d_head, int N, int fh, int fw, const double *anchors, const float *d_targets,
                       int T, double ignore_thres, void *d_work, size_t work_bytes, float *d_losses, float *d_grad_head, void *stream);
int yf_train_head_loss_workspace_bytes_ex(int N, int fh, int fw, int num_anchors, int num_classes, size_t *out);
int yf_train_head_loss_ex(int device, int H, int W, const float *d_head, int N, int fh, int fw, const double *anchors, int num_anchors,
                          int num_classes, const float *d_targets, int T, double ignore_thres, void *d_work, size_t work_bytes,
                          float *d_losses, float *d_grad_head, void *stream);

/* The same loss with the box regressed as ONE IoU-family term per positive cell in place of the reference's four coordinate terms
 * (opt-in; darknet's and yolov5's formulation).  yf_train_head_loss_ex's arguments, then box_kind and lambda_box.
 *   box_kind YF_BOX_REF runs the reference's terms: d_losses, the gradient and the first 6 + C planes are those of
 *   yf_train_head_loss_ex.  YF_BOX_GIOU / _DIOU / _CIOU, per positive cell (mask == 1 after get_target, which is unchanged: same best
 *   anchor, same ignore marks, the last target written to a cell wins), in feature-map units relative to the cell's corner, from the
 *   cell's float32 logits t0..t3 and its float32 anchor (aw, ah), everything widened to double:
 *     predicted box   px = sigmoid(t0), py = sigmoid(t1), pw = exp(clamp(t2, -C, C)) * aw, ph = exp(clamp(t3, -C, C)) * ah with
 *                     C = YF_BOX_WH_CLAMP -- a guard, not a tuning knob (exp(1000) is infinite and the term NaN without it); its
 *                     derivative is 1 on [-C, C] inclusive and 0 outside
 *     target box      tx, ty (the float32 planes), gw = float32(w * fw), gh = float32(h * fh) of the target that wrote tx
 *     with eps = 1e-7, corners b?x1 = x - w / 2 and so on, 1 = predicted, 2 = target:
 *     inter = max(min(b1x2,b2x2) - max(b1x1,b2x1), 0) * max(min(b1y2,b2y2) - max(b1y1,b2y1), 0)
 *     union = pw*ph + gw*gh - inter + eps              iou = inter / union
 *     cw = max(b1x2,b2x2) - min(b1x1,b2x1)             ch likewise
 *     giou = iou - (cw*ch + eps - union) / (cw*ch + eps)
 *     c2 = cw^2 + ch^2 + eps    rho2 = ((b2x1+b2x2-b1x1-b1x2)^2 + (b2y1+b2y2-b1y1-b1y2)^2) / 4
 *     diou = iou - rho2 / c2
 *     v = 4/pi^2 * (atan(gw/(gh+eps)) - atan(pw/(ph+eps)))^2
 *     alpha = v / (v - iou + 1 + eps), a CONSTANT in the backward (yolov5's no_grad)     ciou = iou - (rho2/c2 + v*alpha)
 *   box = (1 / E) * sum over the positive cells of (1 - value), E = N*A*fh*fw: the normalisation of the reference's four terms (means
 *   over all cells of masked values), so the balance against the confidence term stays where it is; 0 without a positive cell.
 *   total = lambda_box * box + conf + cls, conf and cls exactly those of yf_train_head_loss_ex (cls and total NaN without a positive
 *   cell, as there).  lambda_box = 5.0 is the sum of the reference's weights on x, y (2.5) and w, h (2.5); nobody has trained with it.
 *   The term and its derivative are evaluated in double per positive cell and rounded to float32 once, at the gradient store: in
 *   float32 GIoU's enclosing-area term cancels catastrophically for a clamped, huge box.  Non-positive cells get an exact 0 in channels
 *   0..3; channels 4.. are yf_train_head_loss_ex's arithmetic, bit for bit.  No atomic feeds the gradient; five launches, as there.
 *   d_losses float32 [8] = total, box, 0, 0, 0, conf, cls, and in [7] the count of targets the reference cannot index (as above).
 *   d_work: yf_train_head_loss_box_workspace_bytes bytes, 8-byte aligned: double[16] -- [0] the sum of (1 - value), [1..3] zero,
 *   [4..8] as above (YF_BOX_REF: all as above) -- then float32 [8 + C][E]: the 6 + C planes above, bit for bit, then gw and gh (written
 *   for every box_kind, zero at non-positive cells); up to 64 bytes behind them are reserved and not written.
 *   YF_E_INVALID before any launch for everything yf_train_head_loss_ex refuses, a box_kind outside 0..3 and a lambda_box that is
 *   negative or not finite; YF_E_WORKSPACE for a workspace smaller than reported. */
#define YF_BOX_REF 0
#define YF_BOX_GIOU 1
#define YF_BOX_DIOU 2
#define YF_BOX_CIOU 3
#define YF_BOX_WH_CLAMP 10.0
int yf_train_head_loss_box_workspace_bytes(int N, int fh, int fw, int num_anchors, int num_classes, size_t *out);
int yf_train_head_loss_box(int device, int H, int W, const float *d_head, int N, int fh, int fw, const double *anchors, int num_anchors,
                           int num_classes, const float *d_targets, int T, double ignore_thres, void *d_work, size_t work_bytes,
                           float *d_losses, float *d_grad_head, void *stream, int box_kind, double lambda_box);

/* The same loss with yolov5's objectness and class options (opt-in; the six loss keys of its hyp files and its model.gr).
 * yf_train_head_loss_box's arguments, then eight doubles:
 *     obj_pw, cls_pw    BCE positive weight of the objectness / the class term        neutral 1, 1
 *     label_smoothing   eps of yolov5's smooth_BCE                                    neutral 0
 *     fl_gamma          focal exponent gamma                                          neutral 0
 *     fl_alpha          focal alpha (not read while gamma == 0)
 *     obj_iou           yolov5's gr: how far the objectness target follows the IoU    neutral 0
 *     lambda_conf, lambda_cls   the `obj` and `cls` gains (plain factors)             neutral 1, 1
 *   get_target, the masks, the box terms and the normalisations (conf: a mean over all E cells, cls: over C * n_pos) are those of
 *   yf_train_head_loss_box.  Only the BCE element and its targets change.  p is a float32 sigmoid times its mask, as there:
 *     base(p,t,w) = -( w t max(log p, -100) + (1 - t) max(log(1 - p), -100) )
 *     d base / d p = ( -w t (1 - p) + (1 - t) p ) / max((1 - p) p, 1e-12), times (1 - p) p for the logit
 *   (at w = 1 and a 0/1 target these are torch's BCELoss element and backward, the ones yf_train_head_loss_ex uses).
 *   Focal loss, only when gamma > 0 (yolov5's FocalLoss around BCE), on EVERY element of conf_obj, conf_noobj and cls:
 *     p_t = t p + (1 - t)(1 - p)      af = t alpha + (1 - t)(1 - alpha)      elem = base af (1 - p_t)^gamma
 *     the modulating factor is differentiated too: d (1 - p_t)^gamma / d p = gamma (1 - p_t)^(gamma - 1) (1 - 2 t)
 *   0 < gamma < 1 is refused: that derivative is unbounded at p_t = 1.
 *   Positive weights: obj_pw is the w of conf_obj (conf_noobj has target 0, where w is moot), cls_pw the w of cls.
 *   Label smoothing: the class target is cp = float32(1 - 0.5 eps) where the class plane is 1 and cn = float32(0.5 eps) where it is 0
 *   (cp, cn formed in double on the host).  The planes in the workspace stay get_target's 0 / 1; smoothing is applied where they are read.
 *   IoU objectness target: at a positive cell t_obj = float32((1 - g) + g min(max(value, 0), 1)), g = obj_iou, value the cell's GIoU /
 *   DIoU / CIoU value above; a CONSTANT in the backward (yolov5's iou.detach().clamp(0)).  g > 0 with YF_BOX_REF is refused.  A positive
 *   cell whose noobj_mask is still 1 (its best anchor's IoU is not above the ignore threshold) keeps its conf_noobj element, as before.
 *   total = [2.5 (x + y + w + h) or lambda_box * box] + lambda_conf * conf + lambda_cls * cls; d_losses[5] and [6] stay the UNWEIGHTED
 *   conf and cls.  Nobody has trained with any of these options; yolov5's files use fl_gamma 0 or 1.5 and gr 1.
 *   With the neutral values d_losses, the gradient and the whole workspace are those of yf_train_head_loss_box bit for bit, for every
 *   box_kind (the same launches).  Otherwise a term no option touches (conf: obj_pw, gamma, obj_iou; cls: cls_pw, gamma, eps) keeps that
 *   entry's float32 arithmetic, its gradient channels multiplied by the float32 gain; a touched term's elements and derivatives are
 *   evaluated in double on the float32 sigmoid and rounded to float32 once, at the gradient store.  Five launches, no atomic feeds the
 *   gradient, no host synchronisation; d_work and its size are yf_train_head_loss_box's.
 *   YF_E_INVALID before any launch for everything yf_train_head_loss_box refuses, a non-finite option, obj_pw or cls_pw <= 0,
 *   label_smoothing, fl_alpha or obj_iou outside [0, 1], fl_gamma < 0 or in (0, 1), obj_iou > 0 with YF_BOX_REF, a negative gain. */
int yf_train_head_loss_hyp_workspace_bytes(int N, int fh, int fw, int num_anchors, int num_classes, size_t *out);
int yf_train_head_loss_hyp(int device, int H, int W, const float *d_head, int N, int fh, int fw, const double *anchors, int num_anchors,
                           int num_classes, const float *d_targets, int T, double ignore_thres, void *d_work, size_t work_bytes,
                           float *d_losses, float *d_grad_head, void *stream, int box_kind, double lambda_box, double obj_pw, double cls_pw,
                           double label_smoothing, double fl_gamma, double fl_alpha, double obj_iou, double lambda_conf, double lambda_cls);

/* Operators of the reference's TRAINING step (second slice): every layer type of YoloFastest in train mode, forward
 * and backward, on NCHW float32 device tensors like the reference's (src/model_training/model/yolo_fastest.py:16-66, train.py:98-160).
 * Per-layer kernels (MFMA GEMMs for the pointwise / dense convs, split reductions added in a fixed order: DESIGN.md section 4) -- not the
 * tuned inference engine, which folds BatchNorm and therefore cannot train.  `device` = HIP device index; everything is stream-ordered.
 *   conv: Conv2d(k in {1,3,5}, stride in {1,2}, pad (k-1)/2, groups 1 or C [depthwise = 1]); d_w [Cout, Cin/groups, k, k]; d_bias or NULL.
 *   deconv: ConvTranspose2d(k 2, stride 2, pad 0); d_w [Cin, Cout, 2, 2]; output 2H x 2W.
 *   bn: BatchNorm2d in train mode (eps 1e-5, momentum 0.1): d_stats float[2C] receives (mean, invstd) per channel for the backward;
 *       running_mean / running_var are updated in place (unbiased variance) unless NULL; relu = 1 fuses the following ReLU (the backward
 *       then masks by y > 0, with y recomputed from x bit for bit -- it does not read the forward's output).  bn_backward: d_x = the
 *       forward's input, d_dgamma, d_dbeta [C], d_dx like x.  C <= 256.
 *   d_scratch: yf_train_scratch_bytes() of device memory, one per stream, no initialisation needed: the per-channel reductions of bn
 *       and the weight gradients are split over many workgroups that store partial results there, and a second pass adds them in a
 *       fixed order (deterministic; device-scope float atomics are slow on a multi-XCD part).  conv_backward_weight accepts NULL / a
 *       smaller buffer (scratch_bytes) and then splits less.
 *   adam_step: torch.optim.Adam(lr, betas, eps), no weight decay (train.py:84); step counts from 1. */
int yf_train_conv_forward(int device, const float *d_x, const float *d_w, const float *d_bias, float *d_y, int N, int Cin, int H, int W, int Cout,
                          int k, int stride, int depthwise, void *stream);
int yf_train_conv_backward_data(int device, const float *d_dy, const float *d_w, float *d_dx, int N, int Cin, int H, int W, int Cout, int k,
                                int stride, int depthwise, void *stream);
int yf_train_conv_backward_weight(int device, const float *d_x, const float *d_dy, float *d_dw, int N, int Cin, int H, int W, int Cout, int k,
                                  int stride, int depthwise, void *d_scratch, size_t scratch_bytes, void *stream);
int yf_train_deconv_forward(int device, const float *d_x, const float *d_w, float *d_y, int N, int Cin, int H, int W, int Cout, void *stream);
int yf_train_deconv_backward_data(int device, const float *d_dy, const float *d_w, float *d_dx, int N, int Cin, int H, int W, int Cout, void *stream);
int yf_train_deconv_backward_weight(int device, const float *d_x, const float *d_dy, float *d_dw, int N, int Cin, int H, int W, int Cout,
                                    void *d_scratch, size_t scratch_bytes, void *stream);
int yf_train_scratch_bytes(size_t *bytes);
int yf_train_bn_forward(int device, const float *d_x, const float *d_gamma, const float *d_beta, float *d_running_mean, float *d_running_var,
                        float *d_stats, float *d_y, int N, int C, long HW, int relu, void *d_scratch, void *stream);
int yf_train_bn_backward(int device, const float *d_x, const float *d_dy, const float *d_stats, const float *d_gamma, const float *d_beta,
                         float *d_dgamma, float *d_dbeta, float *d_dx, int N, int C, long HW, int relu, void *d_scratch, void *stream);
/* One block of the network each way -- conv_norm_relu / conv_norm / deconv_norm_relu (yolo_fastest.py:16-48): conv (deconv = 1:
 * ConvTranspose2d) + BatchNorm (+ ReLU).  forward: d_z = conv output (kept for the backward), d_y = block output.  backward: d_gy =
 * gradient of the block output -> d_dgamma, d_dbeta, d_dw, d_dx (NULL: not needed, the first layer); d_gz: work tensor like z. */
int yf_train_unit_forward(int device, int deconv, const float *d_x, const float *d_w, const float *d_gamma, const float *d_beta,
                          float *d_running_mean, float *d_running_var, float *d_stats, float *d_z, float *d_y, int N, int Cin, int H, int W, int Cout,
                          int k, int stride, int depthwise, int relu, void *d_scratch, void *stream);
int yf_train_unit_backward(int device, int deconv, const float *d_x, const float *d_z, const float *d_gy, const float *d_stats, const float *d_w,
                           const float *d_gamma, const float *d_beta, float *d_dgamma, float *d_dbeta, float *d_gz, float *d_dw, float *d_dx, int N,
                           int Cin, int H, int W, int Cout, int k, int stride, int depthwise, int relu, void *d_scratch, size_t scratch_bytes,
                           void *stream);
int yf_train_channel_sum(int device, const float *d_dy, float *d_out, int N, int C, long HW, void *stream);                 /* bias gradient */
/* the same sum spread over the chip for large N HW (partial sums in d_scratch, yf_train_scratch_bytes(); a second launch adds them in order) */
int yf_train_channel_sum_split(int device, const float *d_dy, float *d_out, int N, int C, long HW, void *d_scratch, void *stream);
int yf_train_add(int device, const float *d_a, const float *d_b, float *d_out, long total, void *stream);                   /* residual / grad sum */
int yf_train_channel_slice(int device, const float *d_src, float *d_dst, int N, int C, long HW, int Cs, int sc0, int Cd, int dc0,
                           void *stream);                                                                                    /* torch.cat and back */
int yf_train_adam_step(int device, float *d_p, const float *d_g, float *d_m, float *d_v, long total, double lr, double beta1, double beta2,
                       double eps, int step, void *stream);
/* the same update for `ntensors` tensors in one launch: HOST arrays of device pointers and sizes; d_table: >= 48 * ntensors bytes of
 * device scratch (the pointer table is uploaded into it on `stream`). */
int yf_train_adam_multi(int device, int ntensors, void *const *d_p, const void *const *d_g, void *const *d_m, void *const *d_v, const long *sizes,
                        double lr, double beta1, double beta2, double eps, int step, void *d_table, size_t table_bytes, void *stream);
/* ... with a caller-owned PINNED host copy of the table (>= 48 * ntensors bytes, one per optimizer): the table is written there and
 * uploaded asynchronously, and only when `upload` != 0 -- set it when the pointer set changed; before the NEXT call with upload != 0 the
 * previous upload must have executed (wait on an event recorded behind this call).  h_table_pinned NULL = yf_train_adam_multi. */
int yf_train_adam_multi_pinned(int device, int ntensors, void *const *d_p, const void *const *d_g, void *const *d_m, void *const *d_v,
                               const long *sizes, double lr, double beta1, double beta2, double eps, int step, void *d_table, size_t table_bytes,
                               void *h_table_pinned, int upload, void *stream);

/* Every tensor of every param group of an optimizer in ONE launch (training.SGD, training.Adam).  `kind` selects the update:
 *   YF_OPT_SGD   torch.optim.SGD(lr, momentum, weight_decay, nesterov), bit for bit, every scalar rounded once from double to float:
 *                    d = weight_decay != 0 ? fma(weight_decay, p, g) : g
 *                    buf = first[t] ? d : round(momentum * buf) + d          (momentum != 0 only; d_s1[t] is the momentum buffer)
 *                    d = nesterov ? fma(momentum, buf, d) : buf
 *                    p = fma(-lr, d, p)
 *                first[t] != 0 marks a tensor's first step (its buffer is written, not read); first NULL = no tensor is on its first
 *                step.  d_s1 may be NULL when no group has momentum, d_s2 is not read.
 *   YF_OPT_ADAM  torch.optim.Adam(lr, betas, eps, weight_decay) (L2, not AdamW): g' = weight_decay != 0 ? fma(weight_decay, p, g) : g,
 *                then the arithmetic of yf_train_adam_multi (with weight_decay == 0: its bits).  d_s1 = exp_avg, d_s2 = exp_avg_sq,
 *                groups[i].step counts from 1; first is not read.
 * group_of[t] names tensor t's group, 0 .. ngroups-1, ngroups <= YF_OPT_MAX_GROUPS.  The per-group scalars travel as kernel arguments,
 * not in the table: a call that only changes them (the warm-up's per-iteration lr) passes upload == 0.  d_table / h_table_pinned /
 * upload as in yf_train_adam_multi_pinned, with YF_OPT_TABLE_ENTRY_BYTES per tensor; upload != 0 too when group_of or first changed.
 * YF_E_INVALID before the GPU is touched for: a null pointer, a size <= 0, a group index out of range, ngroups outside
 * 1 .. YF_OPT_MAX_GROUPS, dampening != 0, maximize != 0, nesterov without momentum, a negative momentum, Adam step < 1, an unknown kind. */
#define YF_OPT_ADAM 0
#define YF_OPT_SGD 1
#define YF_OPT_MAX_GROUPS 8
#define YF_OPT_TABLE_ENTRY_BYTES 56
typedef struct yf_opt_group {
    double lr, weight_decay;
    double momentum, dampening;         /* SGD; dampening must be 0 */
    double beta1, beta2, eps;           /* Adam */
    int nesterov;                       /* SGD */
    int step;                           /* Adam: this step's number, >= 1 */
    int maximize;                       /* must be 0 */
    int reserved;
} yf_opt_group;
int yf_train_opt_multi_pinned(int device, int kind, int ntensors, void *const *d_p, const void *const *d_g, void *const *d_s1, void *const *d_s2,
                              const long *sizes, const int *group_of, const int *first, int ngroups, const yf_opt_group *groups, void *d_table,
                              size_t table_bytes, void *h_table_pinned, int upload, void *stream);

/* yf_train_opt_multi_pinned with yolov5's ModelEMA kept inside the same launch (training.ModelEMA; step(ema=...)): after tensor t's
 * update the kernel goes on with the value it just stored in p, every scalar rounded once from double to float:
 *                    d_f = (float)d;  omd_f = (float)(1.0 - d)
 *                    a = round(e * d_f)                                      (e: the element of d_ema[t])
 *                    b = round(omd_f * p)                                    (p: the element of d_p[t] as just written)
 *                    e = round(a + b)
 * three separately rounded fp32 operations, never a fused multiply-add: torch's `v *= d; v += (1 - d) * p` on float32 tensors.
 * d_ema: HOST array of `ntensors` device pointers, one per optimised tensor.  The `n_extra` tensors behind them are EMA-only --
 * d_extra_src[t] is read, d_extra_ema[t] gets the three lines above, no gradient and no optimizer arithmetic (BatchNorm running
 * statistics, parameters without a gradient); n_extra == 0 allows the three arrays to be NULL.  d: this update's decay, e.g.
 * decay * (1 - exp(-updates / tau)); d_f and omd_f travel as kernel arguments, so a call that differs only in d passes upload == 0.
 * d_table / h_table_pinned / upload as in yf_train_opt_multi_pinned with YF_OPT_EMA_TABLE_ENTRY_BYTES per tensor, ntensors + n_extra
 * of them; upload != 0 too when an EMA or EMA-only pointer changed.  Stream-ordered, capturable, no allocation, no synchronisation.
 * YF_E_INVALID before the GPU is touched for everything yf_train_opt_multi_pinned refuses, and for: d outside [0, 1] or not finite,
 * n_extra < 0, a null EMA / source pointer, an EMA-only size <= 0, an EMA pointer equal to its source, a table that is too small. */
#define YF_OPT_EMA_TABLE_ENTRY_BYTES 64
int yf_train_opt_ema_multi_pinned(int device, int kind, int ntensors, void *const *d_p, const void *const *d_g, void *const *d_s1,
                                  void *const *d_s2, const long *sizes, const int *group_of, const int *first, int ngroups,
                                  const yf_opt_group *groups, void *const *d_ema, int n_extra, const void *const *d_extra_src,
                                  void *const *d_extra_ema, const long *extra_sizes, double d, void *d_table, size_t table_bytes,
                                  void *h_table_pinned, int upload, void *stream);
/* The average alone, ONE launch for `ntensors` (d_src[t], d_ema[t], sizes[t]) triples (training.ModelEMA.update beside any optimizer):
 *                    e = round(round(e * d_f) + round(omd_f * s))            (s: the element of d_src[t]; d_f, omd_f as above)
 * The table takes YF_EMA_TABLE_ENTRY_BYTES per tensor; d_table / h_table_pinned / upload, the stream ordering and the refusals (null
 * pointer, size <= 0, d outside [0, 1] or not finite, d_ema[t] == d_src[t], table too small) as above. */
#define YF_EMA_TABLE_ENTRY_BYTES 32
int yf_train_ema_multi_pinned(int device, int ntensors, const void *const *d_src, void *const *d_ema, const long *sizes, double d,
                              void *d_table, size_t table_bytes, void *h_table_pinned, int upload, void *stream);

/* The same training forward / backward as ONE call each: the whole graph of yolo_fastest.py:150-218 in train mode (what
 * `pred = model(imgs)` and `loss.backward()` run, train.py:114, :131), launched from C++ into a caller-owned workspace.
 *   d_params / d_grads: HOST arrays of yf_trainer_num_params() device pointers in `model.parameters()` order (per conv block: conv
 *     weight, BN weight, BN bias; per head: weight, bias); d_grads are written, not accumulated.
 *   d_bn_buffers: HOST array of 2 * n_bn device pointers (running_mean, running_var per BatchNorm in module order) or NULL.
 *   d_ws: yf_trainer_workspace_bytes(t, N) bytes; forward leaves the activations there and backward reads them: the same buffer,
 *     untouched in between.  backward also needs the images again (d_x: the first conv's weight gradient).
 * Stream-ordered, no allocation, no synchronisation. */
typedef struct yf_trainer_s *yf_trainer;
int yf_trainer_create(int H, int W, int device, yf_trainer *out);                                       /* input_channel 1, num_out 24 */
int yf_trainer_create_ex(int H, int W, int device, int input_channel, int num_out, yf_trainer *out);   /* yolo_fastest.py:72-78 */
void yf_trainer_destroy(yf_trainer t);
int yf_trainer_num_params(yf_trainer t, int *n_params, int *n_bn);
int yf_trainer_workspace_bytes(yf_trainer t, int N, size_t *bytes);
int yf_trainer_forward(yf_trainer t, const float *d_x, int N, const void *const *d_params, void *const *d_bn_buffers, float *d_head_large,
                       float *d_head_small, void *d_ws, size_t ws_bytes, void *stream);
int yf_trainer_backward(yf_trainer t, const float *d_x, const float *d_grad_head_large, const float *d_grad_head_small, int N,
                        const void *const *d_params, void *const *d_grads, void *d_ws, size_t ws_bytes, void *stream);
/* how many passes ran as a HIP graph replay: a pass whose pointer arguments equal those of the call before it is captured once and
   replayed from then on (the steady state of a training loop); YF_TRAIN_GRAPH_OFF=1 in the environment disables it */
int yf_trainer_graph_replays(yf_trainer t, long *forward, long *backward);
/* out6 = replays (forward, backward), captures (forward, backward), evictions (forward, backward).  A trainer keeps up to four graphs per
   pass (one per remembered pointer set); a pointer pattern that keeps evicting graphs before they were replayed stops capturing. */
int yf_trainer_graph_stats(yf_trainer t, long *out6);
int yf_trainer_set_graphs(yf_trainer t, int on);   /* 0: this trainer issues every pass as plain launches (the environment variable YF_TRAIN_GRAPH_OFF
                                                      does the same for the whole process); default 1 */

/* yf_forward + yf_decode_nms back to back on one stream (heads also returned; may be NULL to use
 * workspace-internal buffers). */
int yf_detect(yf_handle h, const float *d_x, int N, double conf_thres, double nms_thres, const double *anchors,
              int origin_h, int origin_w, int K_max, int32_t *d_boxes, float *d_scores, int32_t *d_cls,
              int32_t *d_src, int32_t *d_counts, float *d_head_large, float *d_head_small, void *d_workspace,
              size_t workspace_bytes, void *stream);

/* yf_detect with the packed record block of yf_decode_nms_packed as its output. */
int yf_detect_packed(yf_handle h, const float *d_x, int N, double conf_thres, double nms_thres, const double *anchors, int origin_h,
                     int origin_w, int K_max, int32_t *d_records, float *d_head_large, float *d_head_small, void *d_workspace,
                     size_t workspace_bytes, void *stream);

/* Detect_YOLO.__pre_process arithmetic on device: d_u8 uint8 [N,src_h,src_w] gray frames ->
 * d_x float32 [N,1,H,W] = (v-128)/255 where v is the pixel itself (src == net size) or the 2x2
 * box mean (a+b+c+d+2)>>2 (src == 2x net size).  Other ratios: YF_E_INVALID.
 * C_in = 3: d_u8 uint8 [N,src_h,src_w,3] as cv2.imread returns a frame (HWC, BGR) -> d_x float32 [N,3,H,W] with the channel order
 * reversed, detect.py:119 `img[:, :, ::-1].transpose(2, 0, 1)`; the box mean is taken per channel. */
int yf_preprocess_u8(yf_handle h, const uint8_t *d_u8, int N, int src_h, int src_w, float *d_x, void *stream);

/* yf_forward on u8 frames: Detect_YOLO.__pre_process's arithmetic (src/detect.py:115-124) in front of the net.  d_u8 uint8 [N,src_h,src_w]
 * (C_in = 3: [N,src_h,src_w,3] HWC BGR) of ANY size (detect.py:115-116: `cv2.resize(img, (input_shape[1], input_shape[0]))`):
 *   src == net size, or exactly 2x (cv::resize turns INTER_LINEAR into INTER_AREA there: the 2x2 box mean (a+b+c+d+2)>>2): fused into the
 *     first kernel's loads -- bit-identical to yf_preprocess_u8 followed by yf_forward, one pass and 3-15 bytes per pixel less HBM traffic;
 *   any other size: one extra pass (yf_cv_preprocess_u8: cv::resize's 8-bit INTER_LINEAR) into net-sized u8 frames at the end of the
 *     workspace, then the fused entry.  The first call for a new source size builds cv::resize's coefficient tables with one small
 *     kernel on `stream` (no allocation or host synchronisation on this path -- yf_create_ex allocates the table pool; 32 distinct
 *     source sizes are kept, a 33rd evicts behind a device synchronisation).  Stream capture: the rules at yf_cv_preprocess_u8. */
int yf_forward_u8(yf_handle h, const uint8_t *d_u8, int N, int src_h, int src_w, float *d_head_large, float *d_head_small,
                  void *d_workspace, size_t workspace_bytes, void *stream);

/* The two OpenCV calls of Detect_YOLO.__pre_process (src/detect.py:110-116) on the device, for any source size:
 *     img = cv2.cvtColor(ori_img, cv2.COLOR_BGR2GRAY)        1-channel net, src_c == 3 (cv2.imread's BGR frames)
 *     img = cv2.resize(img, (W, H))                           INTER_LINEAR; exactly 1/2 -> the 2x2 mean; same size -> copy
 * d_src uint8 [N,src_h,src_w(,3)] -> d_dst uint8 [N,H,W(,C_in)] (a 3-channel net keeps BGR order: detect.py:119's reversal is the next step).
 * OpenCV's published 8-bit arithmetic is restated: gray = (B*BY + G*GY + R*RY + half) >> shift with gray_bits 15 (9798/19235/3735: OpenCV 4.x;
 * 0 means 15) or 14 (4899/9617/1868: OpenCV 2.x / 3.x); resize with 11-bit coefficients, dst = (((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2) >> 2.
 * Bit-exact against oracle/cv_oracle.py; parity with an actual OpenCV build is UNPINNED (cv2 is not available where this was built, and an
 * IPP / vendor-HAL build may round differently).
 *
 * Stream capture (this entry, yf_forward_bgr_u8 and yf_forward_u8 at a source size that is neither the net's nor twice it).  The resize
 * reads per-size coefficient tables out of a pool of 32 slots that the engine owns (allocated and zeroed by yf_create_ex).  A table is
 * built only by an EAGER call; under capture the call refers to a table that exists:
 *   - the first sight of a source size while `stream` is capturing returns YF_E_INVALID ("run once eagerly at this source size before
 *     capturing") and changes nothing: nothing is launched, no slot is taken, the capture stays valid;
 *   - a size seen before is captured once its eager build has finished on the device -- synchronise with that call's stream before the
 *     capture begins; a build still in flight returns YF_E_INVALID -- and its slot is PINNED for the engine's lifetime, because the graph
 *     keeps the slot's addresses.  Replays and eager calls at that size may then be mixed freely, from any stream;
 *   - the 33rd distinct size evicts the least recently used UNPINNED slot; with all 32 slots pinned a new size returns YF_E_INVALID. */
int yf_cv_preprocess_u8(yf_handle h, const uint8_t *d_src, int N, int src_h, int src_w, int src_c, int gray_bits, uint8_t *d_dst, void *stream);

/* yf_forward on cv2.imread's frames (uint8 [N,src_h,src_w,3], BGR) of any size: yf_cv_preprocess_u8 + the fused (v-128)/255 entry.  What
 * `Detect_YOLO.batch_detect` does per image (detect.py:108-127, 152), batched.  A 3-channel net: identical to yf_forward_u8.
 * Stream capture: yf_cv_preprocess_u8's rules (a source size is run once eagerly before it is captured). */
int yf_forward_bgr_u8(yf_handle h, const uint8_t *d_bgr, int N, int src_h, int src_w, int gray_bits, float *d_head_large, float *d_head_small,
                      void *d_workspace, size_t workspace_bytes, void *stream);

/* yolov5's letterbox in front of the net and its scale_boxes behind the NMS (opt-in; the reference squashes every frame to the net's size
 * and scales every box to the CONFIGURED original shape: yf_cv_preprocess_u8, the origin_h / origin_w of yf_decode_nms).
 *
 * The rule.  H, W: the net's input size, C its channels (1 or 3); the frame is uint8 [h, w, 3], BGR.  Geometry is yolov5's
 * letterbox(im, (H, W), auto=False, scaleFill=False, scaleup=True), in IEEE double with Python's round (half to even):
 *     r      = min(H / h, W / w)
 *     new_w  = int(round(w * r));  new_h = int(round(h * r))
 *     dw, dh = (W - new_w) / 2, (H - new_h) / 2
 *     top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1));   left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
 * Pixels, in the reference's order of operations (detect.py:110-116): BGR2GRAY first when C == 1; then cv2.resize(img, (new_w, new_h)) with
 * the arithmetic of yf_cv_preprocess_u8 -- 11-bit INTER_LINEAR, exactly 1/2 in both directions -> the 2x2 mean, same size -> a copy, decided
 * on (h, w) against (new_h, new_w), not against (H, W) --; then cv2.copyMakeBorder(top, bottom, left, right, value=114): every destination
 * byte outside [top, top + new_h) x [left, left + new_w) is 114, in all channels.  A frame of the net's aspect ratio comes out as
 * yf_cv_preprocess_u8's bytes with no border.
 * Boxes come back by yolov5's scale_boxes((H, W), boxes, (h, w)) with ratio_pad=None, then .round(); in double, per coordinate:
 *     gain = min(H / h, W / w);  pad_w = (W - w * gain) / 2;  pad_h = (H - h * gain) / 2
 *     x' = round_half_even(clip((x - pad_w) / gain, 0, w));   y' = round_half_even(clip((y - pad_h) / gain, 0, h))
 * -- yolov5's FLOAT pad, not the integer left / top the pixels were placed with (they differ by less than one source pixel).
 * Not covered: auto=True (the minimal rectangle), scaleFill, scaleup=False.  Training and validation items on letterboxed frames:
 * yf_augment_letterbox_u8 below.
 *
 * yf_letterbox_geometry: host only, never touches a GPU.  out = new_h, new_w, top, bottom, left, right.  YF_E_INVALID for a size <= 0.
 *
 * yf_cv_letterbox_u8: N frames of ANY sizes in ONE launch.  d_frames / heights / widths: HOST arrays of N device pointers (each a
 * contiguous uint8 [h, w, 3] frame with no alignment requirement: its own allocation, a slice of a stack, a view) and their sizes.
 * gray_bits: 0 = the three channels are kept (d_dst [N, dst_h, dst_w, 3], still BGR), 14 | 15 = BGR2GRAY with those coefficients
 * (d_dst [N, dst_h, dst_w]).  The per-frame table (pointer, h, w and the six geometry integers: YF_LB_TABLE_ENTRY_BYTES each) is filled
 * on the host into the caller's PINNED copy and uploaded on `stream` into d_table; as with yf_train_opt_multi_pinned the previous upload
 * from h_table_pinned must have executed before the next call rewrites it (wait on an event recorded behind the call).  Stream-ordered:
 * no allocation, no synchronisation.  The resize coefficients are computed inside the kernel from (h -> new_h, w -> new_w) with the
 * expressions of yf_cv_resize_tables: no table pool, no per-size cache.  Every source index is clamped to the frame; h == 1 and w == 1 are
 * legal.  YF_E_INVALID before any launch for: N <= 0, a null pointer, a size <= 0, a side above 8192, gray_bits outside {0, 14, 15}, a
 * table smaller than N entries, and a frame so thin that new_h or new_w rounds to 0 (cv2.resize raises there too).
 *
 * yf_scale_boxes: one launch, in place.  Rewrites the first min(max(count, 0), K_max) boxes (x1, y1, x2, y2 in net coordinates: the NMS
 * run with origin 0, 0) of every frame by the rule above.  Frame f's boxes start at d_boxes + f * frame_stride, its count is
 * d_counts[f * count_stride] (strides in int32 elements): the separate tensors of yf_decode_nms are (4 K_max, 1), the record block of
 * yf_decode_nms_packed is (1 + 8 K_max, 1 + 8 K_max) with d_boxes = d_records + 1 and d_counts = d_records.  Slots past the count and
 * frames with count -2 are left untouched, as is a frame whose d_frame_hw (device int32 [N, 2]: h, w) entry is not positive. */
#define YF_LB_TABLE_ENTRY_BYTES 40
#define YF_LB_MAX_SIDE 8192
int yf_letterbox_geometry(int src_h, int src_w, int dst_h, int dst_w, int32_t out[6]);
int yf_cv_letterbox_u8(int device, int N, const void *const *d_frames, const int *heights, const int *widths, int gray_bits, int dst_h, int dst_w,
                       uint8_t *d_dst, void *d_table, size_t table_bytes, void *h_table_pinned, void *stream);
int yf_scale_boxes(int device, int32_t *d_boxes, long frame_stride, const int32_t *d_counts, long count_stride, int N, int K_max, int net_h,
                   int net_w, const int32_t *d_frame_hw, void *stream);

/* The image half of the reference's DetectDataset.__getitem__ (src/model_training/dataloader/detect_dataset.py:90-103, :132-143) on the
 * device, handle-free like the training operators (a dataset owns no model), for N same-size source frames in ONE launch:
 *     x = fliplr?(GaussianBlur_k(resize(cvtColor_BGR2GRAY?(frame))))        per frame: k in {0 (none), 3, 5, 7}, flip in {0, 1}
 *   d_src     u8 [n_src, src_h, src_w, src_c] (cv2.imread's BGR for src_c 3); d_index: NULL (output frame n = source frame n, n_src >= N) or
 *             int32 [N] source frame per output frame (an entry outside 0 .. n_src - 1 leaves its output frame untouched)
 *   gray      src_c 3 -> dst_c 1: OpenCV's 8-bit BGR2GRAY with gray_bits 15 (0 means 15) or 14 coefficients; otherwise src_c == dst_c (1 or 3)
 *   resize    same size: none; exactly 2x: the 2x2 mean (INTER_AREA's fast path); any other size: INTER_LINEAR through the tables of
 *             the resize-tables entry below for (src_h, src_w) -> (dst_h, dst_w) (d_xtab, d_ytab; not read otherwise, may be NULL)
 *   blur      OpenCV's 8-bit fixed-point GaussianBlur(ksize k, sigma 0): taps /256 [64 128 64], [16 64 96 64 16], [8 28 56 72 56 28 8],
 *             row pass exact, dst = (sum k_y row_y + 2^15) >> 16, BORDER_REFLECT_101, per channel
 *   d_params  int32 [N]: k | flip << 8 (a k other than 3, 5, 7 means no blur); the flip is applied after the blur
 *   outputs   d_u8 u8 [N, dst_h, dst_w, dst_c] and / or d_x float32 [N, dst_c, dst_h, dst_w] = (v - 128) / 255 (BGR order kept), NULL = not wanted
 * Same bytes as the CPU restatement in tests/ composed with oracle/cv_oracle.py; parity with an actual OpenCV build is UNPINNED.
 * No allocation or synchronisation; stream-ordered. */
int yf_augment_u8(int device, const uint8_t *d_src, int src_h, int src_w, int src_c, const int *d_index, int n_src, int N, const void *d_xtab,
                  const void *d_ytab, int dst_h, int dst_w, int dst_c, int gray_bits, const int *d_params, uint8_t *d_u8, float *d_x, void *stream);
/* yf_augment_u8 with yolov5's geometric augmentation (random_perspective) between the resize and the blur, and a vertical flip at the end:
 *     x = flipud?(fliplr?(GaussianBlur_k(warp?(resize(cvtColor_BGR2GRAY?(frame))))))
 *   warp      Pillow's Image.transform(size, AFFINE | PERSPECTIVE, coefficients, resample=BILINEAR, fillcolor=114), bit for bit: per
 *             destination pixel (x, y), in IEEE double with one rounding per operation (no FMA contraction, correctly rounded division):
 *             xin = x + 0.5, yin = y + 0.5; sx = (a0 xin + a1 yin) + a2, sy = (a3 xin + a4 yin) + a5, PERSPECTIVE: each divided by
 *             (a6 xin + a7 yin) + 1.0; 114 on every channel if sx < 0, sx >= dst_w, sy < 0 or sy >= dst_h; otherwise the bilinear sample of
 *             the resized frame at (sx - 0.5, sy - 0.5) with columns and rows clamped, truncated to uint8.
 *             Pinned to Pillow; OpenCV parity not claimed (cv2.warpAffine / warpPerspective interpolate through fixed-point tables).
 *   d_params  int32 [N]: yf_augment_u8's k | fliplr << 8, and bit 9 flipud, bit 10 warp present, bit 11 perspective (a6, a7 are read);
 *             a frame without bit 10 and bit 9 gets yf_augment_u8's bytes
 *   d_warp    float64 [N, 8]: a0 .. a7 of the output -> input map per frame (read for frames with bit 10)
 *   d_scratch caller-owned u8 [N, dst_h, dst_w, dst_c] (may not overlap an output): the resized frames between the two launches
 * Two launches on `stream` (the resize into the scratch, then warp + blur + flips out of it); the blur's reflect-101 border is taken on
 * the warped image.  No allocation or synchronisation; stream-ordered; capturable. */
int yf_augment_warp_u8(int device, const uint8_t *d_src, int src_h, int src_w, int src_c, const int *d_index, int n_src, int N, const void *d_xtab,
                       const void *d_ytab, int dst_h, int dst_w, int dst_c, int gray_bits, const int *d_params, const double *d_warp,
                       uint8_t *d_scratch, uint8_t *d_u8, float *d_x, void *stream);
/* Training items on LETTERBOXED frames of mixed sizes (opt-in: DetectDataset(letterbox=True)): the ragged twin of yf_augment_warp_u8, the
 * squashing resize replaced by the letterbox of the block above.  The rule, once.  The frame is uint8 [h, w, 3] BGR, the net input
 * H x W x C with C 1 or 3:
 *     x = flipud?(fliplr?(GaussianBlur_k(warp?(letterbox(cvtColor_BGR2GRAY?(frame))))))
 *   letterbox exactly yf_cv_letterbox_u8's: the geometry in double with round-half-even, the 11-bit cv2.resize arithmetic, the copy /
 *             2x2-mean / linear decision on (h, w) against (new_h, new_w), a border of 114
 *   blur, flips, warp: those of yf_augment_u8 / yf_augment_warp_u8, on the WHOLE H x W letterboxed image, border included: the blur
 *             mixes 114 into the image's edge rows and columns and reflects (101) at the H x W bounds, not at the image's; the warp
 *             samples the border as image and fills with the same 114 outside
 *   With every parameter 0 the u8 output is yf_cv_letterbox_u8's bytes: what the net trains on is what it detects on.
 * Labels (host only, dataset.py `_labels`): yolov5's LoadImagesAndLabels.__getitem__, non-mosaic branch, in float64 --
 *     rows  = xyxy2xywh(pixel boxes) / (w, h)                      the frame's OWN size
 *     r = min(H / h, W / w);  new_w, new_h = int(round(w * r)), int(round(h * r));  dw, dh = (W - new_w) / 2, (H - new_h) / 2
 *     xyxy  = xywhn2xyxy(rows, r * w, r * h, padw=dw, padh=dh)     x1 = (r * w) * (xc - bw / 2) + dw, ...
 *     rows' = xyxy2xywhn(xyxy, w=W, h=H, clip=True, eps=1e-3)      corners clipped to [0, W - 1e-3] x [0, H - 1e-3]
 * -- yolov5's FLOAT pad again, not the integer left / top of the pixels.
 * Not covered: auto=True / rectangular batches, scaleFill, scaleup=False, the INTER_AREA choice of yolov5's load_image, HSV; mosaic tiles
 * are letterboxed frames (yolov5's are unpadded), so a tile that is not of the net's aspect ratio brings its 114 bars into the canvas.
 *
 * yf_augment_letterbox_u8: d_frames / heights / widths, gray_bits, the table and its protocol: yf_cv_letterbox_u8's (HOST arrays of N
 * device pointers of any alignment; the 40-byte entries filled into the caller's pinned copy and uploaded on `stream`).
 *   d_params  int32 [N] on the device: yf_augment_warp_u8's bits (k, 8 fliplr, 9 flipud, 10 warp, 11 perspective)
 *   geometric NOT in the argument list one would write first: d_params lives on the device and is not read back, so the caller, who drew
 *             the parameters on the host, says whether any frame carries bit 9 or 10.  0: launch 2 is yf_augment_u8's kernel and bits
 *             9 .. 11 are NOT read (a frame that carries them anyway comes out unflipped and unwarped); nonzero: launch 2 is
 *             yf_augment_warp_u8's second kernel, which honours them.
 *   d_scratch caller-owned u8 [N, dst_h, dst_w, C] (may not overlap an output): the letterboxed frames between the two launches
 *   d_warp    float64 [N, 8]: read with `geometric` only, else may be NULL
 *   outputs   d_u8 u8 [N, dst_h, dst_w, C] and / or d_x float32 [N, C, dst_h, dst_w] = (v - 128) / 255
 * TWO launches on `stream`: yf_cv_letterbox_u8's kernel into d_scratch, then the blur / flip (/ warp) kernel over the scratch as N same-size
 * sources -- the calls yf_cv_letterbox_u8 + yf_augment_u8 (or yf_augment_warp_u8) would make, behind one validation and one table upload.
 * A fused single launch (letterbox staged straight into the blur's LDS tile) was built and measured: not faster, so it went.
 * YF_E_INVALID before any launch, and before the pinned table is written, for everything yf_cv_letterbox_u8 refuses, and for: no output,
 * d_params or d_scratch NULL, `geometric` while d_warp is NULL, rows too wide for the LDS tile.  No allocation or synchronisation;
 * stream-ordered. */
int yf_augment_letterbox_u8(int device, int N, const void *const *d_frames, const int *heights, const int *widths, int gray_bits, int dst_h,
                            int dst_w, const int *d_params, int geometric, const double *d_warp, uint8_t *d_scratch, uint8_t *d_u8,
                            float *d_x, void *d_table, size_t table_bytes, void *h_table_pinned, void *stream);
/* yolov5's mixup over frames that are ALREADY resized (and gray): per output frame the first frame, warped or not, blended with a partner
 * frame under the partner's own warp, then yf_augment_warp_u8's blur and flips on the mixture:
 *     x = flipud?(fliplr?(GaussianBlur_k(mix(warp?(first), warp?(partner), r))))
 *   d_frames  u8 [n_frames, h, w, c], c 1 or 3: what yf_augment_u8 with all-zero parameters writes to its u8 output (source sizes no longer
 *             matter here, so a partner may come from another size group)
 *   d_first   int32 [N]: the frame output n is made of (an entry outside 0 .. n_frames - 1 leaves output frame n untouched)
 *   d_second  int32 [N]: the partner; negative = none (the frame does not pass through the blend: yf_augment_warp_u8's bytes);
 *             an entry >= n_frames leaves output frame n untouched as well.  Nothing is read out of bounds.  The frame itself is allowed.
 *   mix       yolov5's `(im * r + im2 * (1 - r)).astype(np.uint8)` per byte, in IEEE double with one rounding per operation (no FMA, no
 *             rearrangement): trunc((double)a * r + (double)b * (1.0 - r)), clamped to 0 .. 255 before the conversion (no change for
 *             0 <= r <= 1; a NaN gives 0).  Both samples are taken as yf_augment_warp_u8 takes them (Pillow's BILINEAR, fill 114).
 *   d_params  int32 [N]: yf_augment_warp_u8's bits for the first frame and the mixture (k, 8 fliplr, 9 flipud, 10 warp, 11 perspective),
 *             and bit 12 partner warped, bit 13 partner perspective
 *   d_warp    float64 [N, 2, 8]: the coefficients of the first frame and of the partner (each read with its warp bit)
 *   d_ratio   float64 [N]: r (read for frames with a partner)
 *   outputs   as yf_augment_warp_u8's (at least one; may not overlap d_frames)
 * Bad arguments are refused with YF_E_INVALID before the GPU is touched.  ONE launch on `stream`; the blur's reflect-101 border is taken
 * on the mixture.  No allocation or synchronisation; stream-ordered; capturable. */
int yf_augment_mix_u8(int device, const uint8_t *d_frames, int n_frames, int N, int h, int w, int c, const int *d_first, const int *d_second,
                      const int *d_params, const double *d_warp, const double *d_ratio, uint8_t *d_u8, float *d_x, void *stream);
/* yolov5's mosaic over frames that are ALREADY resized (and gray): per output frame four h x w tiles around a centre (xc, yc) on a 2h x 2w
 * canvas of 114s, that canvas warped and cropped back to h x w as yf_augment_warp_u8 warps a frame, then its blur and flips:
 *     x = flipud?(fliplr?(GaussianBlur_k(warp(canvas(TL, TR, BL, BR, xc, yc)))))
 * The canvas is never in memory: each bilinear tap is resolved to one of the four tiles, or to 114.
 *   d_frames  u8 [n_frames, h, w, c], c 1 or 3: what yf_augment_u8 with all-zero parameters writes to its u8 output
 *   d_tiles   int32 [N, 4]: the tiles top-left, top-right, bottom-left, bottom-right.  d_tiles[n][1] < 0: output n is NOT a mosaic but
 *             frame d_tiles[n][0] with yf_augment_warp_u8's bytes (bits 10 / 11 honoured, d_centre not read); otherwise all four are
 *             read.  d_tiles[n][0] outside 0 .. n_frames - 1, or for a mosaic any of the other three, leaves output frame n untouched;
 *             nothing is read out of bounds.  The same frame may appear in several tiles.
 *   d_centre  int32 [N, 2]: (xc, yc); a mosaic whose centre is outside 0 <= xc <= 2w, 0 <= yc <= 2h leaves its output untouched
 *   canvas    yolov5's load_mosaic with s * 2 replaced by 2w / 2h: canvas[y1a:y2a, x1a:x2a] = tile[y1b:y2b, x1b:x2b], else 114, with
 *               TL  a = (max(xc - w, 0), max(yc - h, 0), xc, yc)                  b = (w - (x2a - x1a), h - (y2a - y1a), w, h)
 *               TR  a = (xc, max(yc - h, 0), min(xc + w, 2w), yc)                 b = (0, h - (y2a - y1a), min(w, x2a - x1a), h)
 *               BL  a = (max(xc - w, 0), yc, xc, min(2h, yc + h))                 b = (w - (x2a - x1a), 0, w, min(y2a - y1a, h))
 *               BR  a = (xc, yc, min(xc + w, 2w), min(2h, yc + h))                b = (0, 0, min(w, x2a - x1a), min(y2a - y1a, h))
 *   warp      Pillow's Image.transform((w, h), AFFINE | PERSPECTIVE, coefficients, BILINEAR, fillcolor = 114) of that canvas, in IEEE
 *             double with one rounding per operation as yf_augment_warp_u8: 114 if sx < 0, sx >= 2w, sy < 0 or sy >= 2h; columns and
 *             rows clamped to 2w - 1 / 2h - 1; a footprint on a seam mixes two to four tiles, or a tile and 114
 *   d_params  int32 [N]: yf_augment_warp_u8's bits (k, 8 fliplr, 9 flipud, 10 warp, 11 perspective); for a mosaic bit 10 is not
 *             consulted: it always samples through its coefficients
 *   d_warp    float64 [N, 8]: a0 .. a7 of the output -> canvas map (output -> frame for a frame that is no mosaic, read with bit 10)
 *   outputs   as yf_augment_warp_u8's (at least one; may not overlap d_frames)
 * Bad arguments are refused with YF_E_INVALID before the GPU is touched.  ONE launch on `stream`; the blur's reflect-101 border is taken
 * on the warped image.  No allocation or synchronisation; stream-ordered; capturable. */
int yf_augment_mosaic_u8(int device, const uint8_t *d_frames, int n_frames, int N, int h, int w, int c, const int *d_tiles,
                         const int *d_centre, const int *d_params, const double *d_warp, uint8_t *d_u8, float *d_x, void *stream);
/* cv::resize's INTER_LINEAR tables for one (source, destination) size pair into caller-owned device memory: d_xtab int4 [dst_w],
 * d_ytab int4 [dst_h] (16 bytes each entry).  One small kernel on `stream`, no allocation or synchronisation. */
int yf_cv_resize_tables(int device, int src_h, int src_w, int dst_h, int dst_w, void *d_xtab, void *d_ytab, void *stream);

/* Baseline JPEG decoding on the device (csrc/yf_jpeg_kernels.hip): bit for bit what PIL (libjpeg-turbo, ISLOW IDCT, fancy upsampling)
 * returns for SOF0 / SOF1 8-bit Huffman files with 1 component or 3 (luma sampling 1 or 2 each way, chroma 1 x 1), restart markers and
 * custom tables allowed, up to 8192 x 8192.
 * yf_jpeg_pack: host only.  Parses n files (pointer + byte count each) of ONE size and packs descriptors, tables and entropy-coded bytes
 *   into `host_blob` (caller-owned, `blob_cap` bytes, 256-byte aligned).  host_blob == NULL: only *blob_bytes (and *h, *w) are set.  A file
 *   outside the supported subset (progressive, lossless, arithmetic, 12-bit, 2 or >= 4 components, other sampling, DNL, several scans) or
 *   with a broken header returns YF_E_INVALID; yf_last_error_string() names the frame index and the reason.
 * yf_jpeg_workspace_bytes: device workspace yf_jpeg_decode_u8 needs for that blob.
 * yf_jpeg_decode_u8: d_blob = a device copy of the blob (256-byte aligned); writes d_bgr uint8 [n, h, w, 3] (cv2.imread's BGR order,
 *   4-byte aligned) and d_status int32 [n] (0 = decoded; otherwise flags of corrupt entropy data: 1 bad Huffman code, 2 coefficient index
 *   past 63, 4 data exhausted, 8 restart markers missing or extra; the frame's bytes are then unspecified).  `host_blob` is read for the
 *   launch shapes only.  One memset and three kernels on `stream`: no allocation, no synchronisation, capturable.
 * yf_jpeg_frame_info: info[25] = ncomp, colour (0 gray, 1 YCbCr, 2 RGB), MCUs per row, MCU rows, MCUs, blocks per MCU, restart interval,
 *   then per component (3, zeros past ncomp): h, v, blocks per row, block rows (MCU-padded), downsampled width, downsampled height.
 * yf_jpeg_huff_lookup: the decoder's lookup of a 16-bit window (code left-aligned) in table `table` (0..3 DC, 4..7 AC) of frame `frame`:
 *   *length 0 = no code matches.
 *
 * Progressive files (SOF2, opt-in): 8-bit, Huffman, the same component layouts, at most 256 scans, a complete progression (every
 * coefficient of every component coded down to Al = 0: libjpeg smooths blocks otherwise and PIL's pixels are then not the IDCT of the
 * coefficients).  A progressive frame costs more device time than its baseline twin: its scans are serial chains.
 * yf_jpeg_pack_ex: yf_jpeg_pack with `flags`.  0: exactly yf_jpeg_pack.  YF_JPEG_PROGRESSIVE: SOF2 files are accepted too, baseline
 *   and progressive files of one size may share a call.  Every SOS and the DHT / DQT / DRI segments between scans are parsed (each scan
 *   keeps a snapshot of the Huffman tables it names; a component's quantisation table is the one defined when the first scan names it, as
 *   libjpeg latches it), and the scan script is checked: a malformed or incomplete one is refused with YF_E_INVALID like any other file.
 *   yf_jpeg_workspace_bytes and yf_jpeg_decode_u8 take either kind of blob (the blob header says which frames are progressive);
 *   yf_jpeg_decode_u8 then launches jpeg_prog_entropy_kernel for the progressive frames (status flags as above, OR-ed over a frame's
 *   scans; flag 2 = coefficient index past the scan's band).
 * yf_jpeg_scan_info: info[12] for scan `scan` (file order) of frame `frame`: scans of the frame (0: a baseline frame, the rest is zero),
 *   dependency levels, then of the scan: components, component mask (bit c = component c), Ss, Se, Ah, Al, dependency level (1 + the
 *   highest level of an earlier scan that shares a component and overlaps its band, DC = band 0..0; 0 without one: scans of one level
 *   are decoded at the same time), offset in the file and length of its entropy-coded bytes, restart interval.
 * yf_jpeg_huff_lookup_ex: yf_jpeg_huff_lookup in the snapshot that scan `scan` of a progressive frame took of table `table`
 *   (scan < 0: yf_jpeg_huff_lookup). */
#define YF_JPEG_PROGRESSIVE 1
int yf_jpeg_pack(int n, const void *const *files, const size_t *nbytes, void *host_blob, size_t blob_cap, size_t *blob_bytes, int *h, int *w);
int yf_jpeg_workspace_bytes(const void *host_blob, size_t *bytes);
int yf_jpeg_decode_u8(int device, const void *host_blob, const void *d_blob, void *d_workspace, size_t ws_bytes, uint8_t *d_bgr, int *d_status,
                      void *stream);
int yf_jpeg_frame_info(const void *host_blob, int frame, int *info, int n_info);
int yf_jpeg_huff_lookup(const void *host_blob, int frame, int table, unsigned bits16, int *length, int *symbol);
int yf_jpeg_pack_ex(int n, const void *const *files, const size_t *nbytes, int flags, void *host_blob, size_t blob_cap, size_t *blob_bytes,
                    int *h, int *w);
int yf_jpeg_scan_info(const void *host_blob, int frame, int scan, int *info, int n_info);
int yf_jpeg_huff_lookup_ex(const void *host_blob, int frame, int scan, int table, unsigned bits16, int *length, int *symbol);

/* Baseline JPEG encoding on the device (csrc/yf_jpeg_enc_kernels.hip): byte for byte the file PIL (libjpeg-turbo) writes for
 * Image.save(f, "JPEG", quality=q, subsampling=s) without optimize / progressive: Annex K Huffman tables, no restart markers.
 * yf_jpeg_enc_setup: host only.  The header libjpeg writes, the scaled quantisation tables and the geometry for frames of h x w
 *   (1 .. 8192 each) with `channels` 1 (gray) or 3, `quality` 1 .. 100 and `subsampling` 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0) (PIL's numbers;
 *   ignored for gray), written to host_blob (call with host_blob = NULL to get the size).  YF_E_INVALID for anything else and for frames
 *   whose worst-case entropy-coded stream would exceed 2^31 bits (bit offsets are 32-bit).
 * yf_jpeg_enc_info: info[10] = h, w, channels, luma h and v sampling, quality, header bytes, blocks per frame, blocks per MCU, blob bytes;
 *   header (up to 640 bytes), divisors [2][64] (8 * q, natural order) and reciprocals [2][64] where the pointers are not NULL.
 * yf_jpeg_enc_workspace_bytes: device workspace yf_jpeg_encode_u8 needs for n frames (worst-case code lengths: about 5 bytes per sample).
 * yf_jpeg_encode_u8: d_frames uint8 [n, h, w, 3] (bgr = 1: in BGR order as the decoder writes them, 0: RGB) or [n, h, w]; writes frame
 *   f's complete file to d_out + f * stride, its byte count to d_lengths[f] and 0 to d_status[f].  A file that does not fit `stride`
 *   bytes: d_status[f] = 1, d_lengths[f] = the stride it needs, and no byte of its slot is written.  Stream-ordered, no allocation, no
 *   synchronisation, capturable; the blob is read on the host during the call only (it travels as a launch argument).
 * yf_draw_boxes_u8: plot_one_box (plot.py) for every record, in place on d_frames uint8 [n, h, w, 3].  d_rec_begin int32 [n + 1]: frame
 *   f applies records [d_rec_begin[f], d_rec_begin[f + 1]) in order.  A record is 32 int32: five rectangles (x0, y0, x1, y1) inclusive and
 *   clipped to the frame (x1 < x0: none), the colour and the text ink (byte k = channel k in the frames' memory order), the label mask's
 *   x, y, width, height and offset into d_atlas (width 0: none), padding.  The mask is blended as PIL blends text:
 *   t = d * (255 - m) + ink * m + 128, ((t >> 8) + t) >> 8. */
int yf_jpeg_enc_setup(int h, int w, int channels, int quality, int subsampling, void *host_blob, size_t blob_cap, size_t *blob_bytes);
int yf_jpeg_enc_info(const void *host_blob, int *info, int n_info, uint8_t *header, uint16_t *divisors, uint32_t *reciprocals);
int yf_jpeg_enc_workspace_bytes(const void *host_blob, int n, size_t *bytes);
int yf_jpeg_encode_u8(int device, const void *host_blob, const uint8_t *d_frames, int n, int bgr, void *d_workspace, size_t ws_bytes,
                      uint8_t *d_out, size_t stride, int *d_lengths, int *d_status, void *stream);
int yf_draw_boxes_u8(int device, uint8_t *d_frames, int n, int h, int w, const int *d_rec_begin, const int *d_records, const uint8_t *d_atlas,
                     void *stream);

/* Introspection used by tests / bench. */
/* Name ("conv1_8+conv1_9+conv2_1"), layer-granular algorithmic bytes and flops per frame of launch `op` of the
 * current plan (each conv of the op reads its input and writes its output once, + residual read: SURVEY.md 8d). */
int yf_op_info(yf_handle h, int op, char *name, int name_len, double *algorithmic_bytes_per_frame, double *flops_per_frame);
/* The same with the flops split by the pipe they run on in this plan: matrix cores (pointwise / dense / deconv layers of the
 * MFMA kernels) and vector ALU (depthwise convs, the small-channel VALU block kernels).  bench.py prices each against its peak. */
int yf_op_info_ex(yf_handle h, int op, char *name, int name_len, double *algorithmic_bytes_per_frame, double *mfma_flops_per_frame,
                  double *valu_flops_per_frame);
/* Arithmetic the kernel of launch `op` runs in: 0 fp32, 1 fp16 storage + fp16 MFMA, 2 fp32 storage + split-operand fp16 MFMA (a
 * dtype-2 engine runs the launches that have no split-operand kernel in exact fp32: same storage, same accuracy class). */
int yf_op_dtype(yf_handle h, int op, int *kernel_dtype);
/* Kernel dispatches launch `op` issues at batch N: 1, except a chained residual launch at small batches, which is issued block by block
 * (DESIGN.md section 4 "Small batches").  Counter tools that match rocprofv3's dispatch rows to launches by order need it. */
int yf_op_dispatches(yf_handle h, int op, int N, int *dispatches);
/* Kernel dispatches decode + NMS issue for N frames with room for K_max survivors each, under the present yf_set_post_split mode: 2 where
 * the per-(frame, class) form runs (post_split_kernel + the assembly launch), 1 for one workgroup per frame (also the fall-back above 64
 * classes, whatever the mode). */
int yf_post_dispatches(yf_handle h, int N, int K_max, int *dispatches);
/* One forward pass (whole batch in one pass) with a HIP event recorded on `stream` around every launch; blocks until
 * the pass is done and returns each launch's duration in ms in op_ms[yf_num_launches]. */
int yf_profile_forward(yf_handle h, const float *d_x, int N, void *d_workspace, size_t workspace_bytes, void *stream,
                       float *op_ms, int n_ops);
/* the same pass from u8 frames (yf_forward_u8's input conventions): the first launch then includes the fused pre-process */
int yf_profile_forward_u8(yf_handle h, const uint8_t *d_u8, int N, int src_h, int src_w, void *d_workspace, size_t workspace_bytes,
                          void *stream, float *op_ms, int n_ops);
int yf_streams_overlap(yf_handle h, void *stream_a, void *stream_b, int *overlap);
                                                   /* do two HIP streams run concurrently?  The runtime multiplexes streams onto a few
                                                      hardware queues; two on one queue execute strictly in issue order (measured: -30 %
                                                      for two lanes, no gain from two batches in flight).  Host-blocking probe (~0.2 ms:
                                                      a 100 us spin kernel on each); the engine uses it to pick its lane / branch streams
                                                      per caller stream, BatchPipeline to pick the streams of the batches in flight */
int yf_set_profile_repeats(yf_handle h, int repeats);
                                                   /* yf_profile_forward[_u8]: every launch is issued `repeats` (1 .. 64, default 1) times back to
                                                      back between its two events and the elapsed time divided by it -- an event pair around ONE
                                                      launch also times the event packets and the dispatch gap (5-7 us per launch, host dependent:
                                                      rocprofv3's kernel durations are that much shorter); every launch writes its whole output
                                                      from inputs it does not modify, so repeating it changes nothing */
int yf_profile_head_offsets(yf_handle h, int N, size_t *large_off, size_t *small_off);
                                                   /* byte offsets inside the workspace handed to yf_profile_forward[_u8] at which that pass left its
                                                      head logits (NCHW fp32, [N, num_out, H/16, W/16] and [N, num_out, H/32, W/32]): tests hold the
                                                      profiled (repeated-launch) pass itself to yf_forward's bits */
int yf_num_launches(yf_handle h, int *out);       /* kernel launches one yf_forward issues            */
int yf_set_chunk(yf_handle h, int frames);        /* frames per pass of the layer chain (0 = whole batch) */
int yf_set_split_sums(yf_handle h, int on);       /* 1 (default): at a handful of frames (<= 9, fp32 engines, 320x256 nets) the stride-32 residual chain and the
                                                      small head split their channel sums over several workgroups and add the partial sums in chunk order at
                                                      launch boundaries (batch-1 latency: DESIGN.md section 4 "Small batches").  Since round 6 the large-batch
                                                      kernels form the same per-chunk partial sums in the same order: THE SAME BITS either way, a frame's logits
                                                      never depend on how many frames travel with it.  0: the one-workgroup launches at every batch size. */
int yf_set_post_split(yf_handle h, int mode);      /* decode + NMS as one workgroup per frame AND class instead of one per frame (the reference runs NMS per class,
                                                      detect.py:158-169: independent work; a second small launch concatenates the classes in class order) --
                                                      the same records bit for bit, for DENSE frames: 64 frames of 1200 candidates use 192 CUs instead of 64
                                                      (0.127 -> 0.058 ms).  0 (default): automatically when the caller reserves K_max >= 256 survivors per frame,
                                                      the model has <= 8 classes and 2 N <= #CU; 1: always (<= 64 classes); 2: never.  The first dense call of a
                                                      size allocates the engine's scratch (not inside a stream capture). */
int yf_set_lanes(yf_handle h, int lanes);          /* 1..4: chunks of the batch (yf_set_chunk) run on this many concurrent
                                                     streams, forked from / joined to the caller's stream by events    */
int yf_set_branches(yf_handle h, int on);         /* 1 (default): the small head's launches (conv5_3 .. head_5) run on a side stream of
                                                     their lane, beside the large head's (deconv5_1 .. head_4); 0 = in line */
int yf_set_fusion(yf_handle h, int level);        /* 2 (default) = block-fused kernels + the per-frame deep stage's launch boundaries
                                                     removed (conv5_2 in the res5 launch, the small head one launch, deconv5_1 +
                                                     conv4_1_1 one launch); 1 = block-fused kernels (bitwise the same heads);
                                                     0 = one launch per layer, every named tensor probe-able (bring-up / parity) */

/* yolov5's autoanchor (utils/autoanchor.py: check_anchors' metric, kmean_anchors' anchor_fitness and its evolution loop) on label shapes
 * that stay on the device.  Not in the reference.  No engine; anchors.py is the caller.
 *   wh float32 [n,2]: label (w, h) in net-input pixels, each in [0, 2^15).  k float32 [A,2]: anchors, finite and positive.
 *   thr in [1, 256]; t = (float)(1.0 / thr) -- torch compares its float32 tensor with the Python scalar 1 / thr in float32.
 *   Metric, per (label, anchor), all IEEE float32: rw = w / aw, rh = h / ah, x = min(min(rw, 1 / rw), min(rh, 1 / rh)); best = the max of
 *       x over the anchors.  1 / r is a second correctly rounded division of the QUOTIENT: aw / w and w * (1 / aw) round differently and
 *       are not the rule.  A zero side gives x = 0.
 *   Sums, exact integers, so that nothing depends on the order of execution:
 *       cnt_best = #{labels: best > t};   cnt_x = sum over labels of #{anchors: x > t};
 *       fit = sum over the labels with best > t of best * 2^(23+m), m the smallest integer with 2^-m <= t (m <= 8).  A float32 at or
 *       above 2^-m is an integer multiple of 2^-(23+m), so every term is an exact integer <= 2^31 and, n being an int, the sum fits 64 bits.
 *       yolov5's bpr = cnt_best / n, aat = cnt_x / n, anchor_fitness = fit / (n * 2^(23+m)) -- yolov5 forms that mean in float32, and
 *       its value depends on torch's summation order; DECISIONS here compare the integer fit only.
 *   Evolution, yolov5's loop with the mutation table as an INPUT: k float64 [A,2], f = fit((float)k).  For g = 0 .. gen-1 in turn:
 *       kg = max(k * v[g], 2.0) in double, fg = fit((float)kg); if fg > f (strict) then k = kg, f = fg.  The entry scores
 *       YF_ANCHOR_BATCH consecutive generations against the current k in one pass over the labels and accepts the FIRST that improves;
 *       the generations behind it are scored again against the new k in the next pass, so k, f and the accepted set are exactly the
 *       sequential chain's.
 *   k-means -- this library's definition, not scipy's (whose sequential float32 means a parallel sum cannot reproduce):
 *       q int32 [n,2] = rint(wh * 64), quantised once by the caller; s = two doubles, the float32 wh.std(0) yolov5 whitens by.  An
 *       observation is o = ((double)q / 64.0) / s; the squared distance to a centroid c is (o_w - c_w)^2 + (o_h - c_h)^2 in double, every
 *       operation rounded on its own; a label goes to the nearest centroid, the lowest index on ties.  Per cluster the exact 64-bit
 *       sums of q_w, q_h and the count are kept; the new centroid is ((double)sum / (64.0 * count)) / s.  Restart r starts from the
 *       observations of the label rows init[r][0..A).  All R restarts run in lock step, one pass over the labels per iteration.  A
 *       restart stops after the pass whose (sums, count) triples all equal those of its previous pass, or after max_iter passes; its
 *       centroids are those of its last pass' sums, and iters_out[r] = the passes it ran.  A restart that ever has an empty cluster, or
 *       whose de-whitened centroids (float)(c * s) are not all finite and positive, is discarded: iters_out[r] = -1.  The winner is
 *       the surviving restart whose de-whitened centroids have the greatest fit, the earliest on ties (yolov5 lets scipy pick by
 *       distortion instead); k_out = its c * s in double, not sorted.  winner_out = -1 when no restart survives; k_out is then not written.
 *   yf_anchor_metric: S anchor sets d_anchors float32 [S,A,2] in one launch; d_out uint64 [S,3] = (fit, cnt_best, cnt_x) per set.
 *       Stream-ordered, no allocation, no synchronisation.
 *   yf_anchor_evolve: k0, v, k_out, fit_out and accepted_out (int32 [gen]: 1 where generation g was accepted, else 0; may be NULL) are HOST
 *       memory; d_work: yf_anchor_evolve_work_bytes(A) bytes of device scratch, 8-byte aligned.  It SYNCHRONISES on `stream` once per pass
 *       (1 + at most gen passes; about a tenth of gen on yolov5's draws) and must not be called inside a stream capture.
 *   yf_anchor_kmeans: s, init (int32 [R,A], label rows), k_out, winner_out, iters_out (int32 [R]) are HOST memory; d_wh = the same labels
 *       as float32, for the winner's fit; d_work: yf_anchor_kmeans_work_bytes(R, A) bytes, 8-byte aligned.  It synchronises once per
 *       iteration and once for the fit.
 *   The kernels hold one label per lane and the candidates in LDS; partial sums cross workgroups as 64-bit integer vector atomics on
 *   accumulators the entry zeroes in-stream.  No workgroup waits on another; the launch boundary is the only exchange.
 *   YF_E_INVALID before any launch: a null pointer, n < 1, A < 1 or > YF_ANCHOR_MAX_A, S < 1, R < 1, S * A or R * A or YF_ANCHOR_BATCH * A
 *   above 1024, thr outside [1, 256] or NaN, gen < 1, max_iter < 1, an init row outside [0, n), s or an anchor of k0 not finite and positive,
 *   a mutation factor that is not finite; YF_E_WORKSPACE: work_bytes below the helper's value (the helpers return 0 for arguments refused
 *   here).  Arrays that live on the device cannot be inspected without a synchronisation: yf_anchor_check_host checks HOST copies --
 *   wh float32 [n,2] (n may be 0), anchors float32 [num_anchors,2] (may be 0) -- and returns YF_E_INVALID for a label side that is
 *   negative, not finite or >= 2^15 and for an anchor side that is not finite and positive; anchors.py calls it before every upload.
 *   Values it would refuse make the sums meaningless but no access out of bounds. */
#define YF_ANCHOR_BATCH 32   /* generations yf_anchor_evolve scores per pass */
#define YF_ANCHOR_MAX_A 32   /* anchors per set */
int yf_anchor_check_host(const float *wh, int n, const float *anchors, int num_anchors);
int yf_anchor_metric(int device, const float *d_wh, int n, const float *d_anchors, int S, int A, double thr, uint64_t *d_out, void *stream);
size_t yf_anchor_evolve_work_bytes(int A);
int yf_anchor_evolve(int device, const float *d_wh, int n, const double *k0, const double *v, int A, int gen, double thr, void *d_work,
                     size_t work_bytes, double *k_out, uint64_t *fit_out, int32_t *accepted_out, void *stream);
size_t yf_anchor_kmeans_work_bytes(int R, int A);
int yf_anchor_kmeans(int device, const int32_t *d_q, int n, const double *s, const int32_t *init, int R, int A, int max_iter, double thr,
                     const float *d_wh, void *d_work, size_t work_bytes, double *k_out, int32_t *winner_out, int32_t *iters_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
