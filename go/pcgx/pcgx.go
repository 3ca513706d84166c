// Package pcgx binds libpcgx.so (include/pcgx.h), the MI355X hot path, behind
// seqsense/pcgol's interfaces: storage.Search, filter.Filter, icp.Evaluator.
//
// The reference's package surface over this binding -- kdtree.New, voxelgrid.New / WithChunkSize,
// icp.NearestPointCorresponder / PointToPointEvaluator / PointToPointICPGradient under their own names and
// signatures -- is in ../pc/storage/kdtree, ../pc/filter/voxelgrid, ../pc/registration/icp.
//
// NOT compiled in the build image (no Go toolchain there); see go/README.md.
package pcgx

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -lpcgx
#include <stdlib.h>
#include "pcgx.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"math"
	"runtime"
	"sync/atomic"
	"unsafe"

	"github.com/seqsense/pcgol/mat"
	"github.com/seqsense/pcgol/pc"
	"github.com/seqsense/pcgol/pc/filter"
	"github.com/seqsense/pcgol/pc/registration/icp"
	"github.com/seqsense/pcgol/pc/storage"
)

// (import path of this package: github.com/seqsense/pcgol/gpu/pcgx, go/go.mod)

// ErrOutOfRange is returned where the pure-Go filter would panic with
// "index out of range" (pc/filter/voxelgrid/voxelgrid.go:151).
var ErrOutOfRange = errors.New("pcgx: point outside the dense voxel grid")

// ErrNeedsDevice: a sharded Fit was asked of an evaluator that cannot run on the device (a WeightFn closure, a
// Corresponder of the caller's own).
var ErrNeedsDevice = errors.New("pcgx: this evaluator cannot run on the device (WeightFn closure or foreign Corresponder)")

// singlePointCalls counts KDTree.Nearest / Range calls for ONE point: each is a blocking GPU call (tens of
// microseconds), so a loop over them -- the reference's own correspondence.go:25-36, regiongrowing.go:26,47 -- is
// slower than the CPU tree.  Tests of callers that were moved to the batch seams assert the counter stays put.
var singlePointCalls int64

// SinglePointCalls returns how many single-point Nearest / Range calls this process has made.
func SinglePointCalls() int64 { return atomic.LoadInt64(&singlePointCalls) }

func lastError() string {
	buf := make([]byte, 512)
	C.pcgx_last_error((*C.char)(unsafe.Pointer(&buf[0])), C.size_t(len(buf)))
	for i, b := range buf {
		if b == 0 {
			return string(buf[:i])
		}
	}
	return string(buf)
}

// status maps pcgx_status onto the reference's sentinel errors so that
// errors.Is keeps working for callers.
func status(rc C.pcgx_status) error {
	switch rc {
	case C.PCGX_OK:
		return nil
	case C.PCGX_E_NO_POINT:
		return errors.New("no point") // pc/minmax.go:11
	case C.PCGX_E_NOT_ENOUGH_PAIRS:
		return icp.ErrNotEnoughPairs // icp/evaluator.go:16
	case C.PCGX_E_NEED_GRADIENT:
		return icp.ErrNeedGradient // icp/icp.go:15
	case C.PCGX_E_BAD_FIELD:
		return errors.New("invalid field name") // pc/pointcloud.go:115
	case C.PCGX_E_OUT_OF_RANGE:
		return ErrOutOfRange
	default:
		// callers hold the OS thread (runtime.LockOSThread) from the cgo call to here: the C side
		// keeps the message per thread
		return fmt.Errorf("pcgx: %s (status %d)", lastError(), int(rc))
	}
}

// Init selects the GPU of this process (one process per GPU).
func Init(device int) error { return status(C.pcgx_init(C.int32_t(device))) }

func init() {
	// the struct layouts this file was compiled against (include/pcgx.h) must be the library's
	if v := int(C.pcgx_abi_version()); v != C.PCGX_ABI_VERSION {
		panic(fmt.Sprintf("pcgx: libpcgx.so speaks ABI version %d, this package was built against %d", v, int(C.PCGX_ABI_VERSION)))
	}
}

// xyzLayout finds stride and xyz byte offset of a cloud exactly as
// PointCloud.Vec3Iterator does (pc/pointcloud.go:130-150).
func xyzLayout(pp *pc.PointCloud) (stride, off int, err error) {
	state, start := 0, 0
	for i, name := range pp.Fields {
		switch {
		case name == "xyz":
			return pp.Stride(), off, nil
		case name == "x" && state == 0:
			state, start = 1, off
		case name == "y" && state == 1:
			state = 2
		case name == "z" && state == 2:
			return pp.Stride(), start, nil
		default:
			state = 0
		}
		off += pp.Size[i] * pp.Count[i]
	}
	return 0, 0, errors.New("invalid field name")
}

// ---------------------------------------------------------------- KD-tree

// KDTree implements storage.Search on the GPU (replaces kdtree.New /
// KDTree.Nearest, pc/storage/kdtree/kdtree.go:33-56,83-146).
type KDTree struct {
	pc.Vec3RandomAccessor
	t *devTree // shared by the shallow copies With() makes (kdtree.go:58-65)
	// MinDistSq > 0 selects the reference's approximate search (kdtree.go:20-22).
	MinDistSq float32
}

// devTree owns the device handle; the copies of a KDTree share it, the last one garbage-collected (or the
// first Close) releases it.
type devTree struct {
	h *C.pcgx_kdtree
}

// KDTreeOption mirrors kdtree.KDTreeOption (kdtree.go:31): New(ra, opts...) and (*KDTree).With(opts...)
// apply them to the tree value exactly as the reference does.  The reference defines no option of its
// own (its one knob is the exported field MinDistSq); WithMinDistSq is the option form of that field.
type KDTreeOption func(*KDTree)

// WithMinDistSq sets KDTree.MinDistSq (kdtree.go:20-22).
func WithMinDistSq(d float32) KDTreeOption { return func(k *KDTree) { k.MinDistSq = d } }

var _ storage.Search = (*KDTree)(nil)

// cloudLayout says where a Vec3RandomAccessor's points already lie packed in memory, so that New can
// hand the caller's bytes to pcgx_kdtree_build as they are (data, stride, xyz offset -- the record layout
// of pc/pointcloud.go:64-78) instead of copying them out through n Vec3At interface calls: at 1M points
// that loop costs more than the 2.5 ms device build.
func cloudLayout(ra pc.Vec3RandomAccessor) (data unsafe.Pointer, stride, off int, keep interface{}, ok bool) {
	switch v := ra.(type) {
	case pc.Vec3Slice: // pc/vec3slice.go:8-20: []mat.Vec3, 12-byte records
		if len(v) == 0 {
			return nil, 12, 0, nil, true
		}
		return unsafe.Pointer(&v[0]), 12, 0, v, true
	}
	return nil, 0, 0, nil, false
}

// New builds the tree (kdtree.New, kdtree.go:33-56).  A pc.Vec3Slice is uploaded straight from its own
// memory (NewFromPointCloud does the same for a cloud's records); any other Vec3RandomAccessor through one
// packed copy.
func New(ra pc.Vec3RandomAccessor, opts ...KDTreeOption) (*KDTree, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	n := ra.Len()
	data, stride, off, keep, ok := cloudLayout(ra)
	if !ok {
		xyz := packVec3(ra)
		stride, off, keep = 12, 0, xyz
		if n > 0 {
			data = unsafe.Pointer(&xyz[0])
		}
	}
	t := &devTree{}
	rc := C.pcgx_kdtree_build(data, C.int64_t(n), C.int32_t(stride), C.int32_t(off), &t.h)
	runtime.KeepAlive(keep)
	if err := status(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(t, func(t *devTree) { t.release() })
	k := &KDTree{Vec3RandomAccessor: ra, t: t}
	for _, o := range opts {
		o(k)
	}
	return k, nil
}

// NewFromPointCloud builds the tree over a cloud's points straight from its records (Data, stride and xyz
// offset as PointCloud.Vec3Iterator finds them, pc/pointcloud.go:130-163): what kdtree.New(it) does for
// it, _ := pp.Vec3Iterator(), without reading the cloud point by point.  The tree's accessor is that iterator.
func NewFromPointCloud(pp *pc.PointCloud, opts ...KDTreeOption) (*KDTree, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	it, err := pp.Vec3Iterator()
	if err != nil {
		return nil, err
	}
	stride, off, err := xyzLayout(pp)
	if err != nil {
		return nil, err
	}
	var data unsafe.Pointer
	if pp.Points > 0 {
		data = unsafe.Pointer(&pp.Data[0])
	}
	t := &devTree{}
	rc := C.pcgx_kdtree_build(data, C.int64_t(pp.Points), C.int32_t(stride), C.int32_t(off), &t.h)
	runtime.KeepAlive(pp)
	if err := status(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(t, func(t *devTree) { t.release() })
	k := &KDTree{Vec3RandomAccessor: it, t: t}
	for _, o := range opts {
		o(k)
	}
	return k, nil
}

// With creates a shallow copy of the tree with the options applied (kdtree.go:58-65); the copy shares
// the device tree.
func (k *KDTree) With(opts ...KDTreeOption) *KDTree {
	k2 := *k
	for _, o := range opts {
		o(&k2)
	}
	return &k2
}

func (t *devTree) release() {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	runtime.SetFinalizer(t, nil)
	if t.h != nil {
		C.pcgx_kdtree_free(t.h)
		t.h = nil
	}
}

// Close releases the device tree now (for every copy made by With) instead of at garbage collection.
func (k *KDTree) Close() {
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	if k.t != nil {
		k.t.release()
	}
}

// DeletePoint removes a point from the tree (KDTree.DeletePoint, kdtree.go:322-332).
func (k *KDTree) DeletePoint(pID int) error {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	id := C.int64_t(pID)
	rc := C.pcgx_kdtree_delete_points(k.t.h, &id, 1)
	if rc == C.PCGX_E_OUT_OF_RANGE {
		return fmt.Errorf("%d does not correspond to any point in the tree", pID) // kdtree.go:324
	}
	return status(rc)
}

// NearestBatch is the batched seam: result i equals k.Nearest(q[i], maxRange).
func (k *KDTree) NearestBatch(q []mat.Vec3, maxRange float32) ([]storage.Neighbor, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	n := len(q)
	out := make([]storage.Neighbor, n)
	if n == 0 {
		return out, nil
	}
	ids := make([]int64, n)
	dsq := make([]float32, n)
	rc := C.pcgx_kdtree_nearest_batch(k.t.h, (*C.float)(unsafe.Pointer(&q[0])), C.int64_t(n),
		C.float(maxRange), C.float(k.MinDistSq), (*C.int64_t)(unsafe.Pointer(&ids[0])), (*C.float)(unsafe.Pointer(&dsq[0])))
	if err := status(rc); err != nil {
		return nil, err
	}
	for i := range out {
		out[i] = storage.Neighbor{ID: int(ids[i]), DistSq: dsq[i]}
	}
	return out, nil
}

// Normals estimates a unit surface normal for every point of the tree from its radius neighbourhood
// (extension: no reference parity; include/pcgx.h, pcgx_kdtree_normals).  The result is in the tree's id
// order: the base normals of the point-to-plane extension.  A degenerate point (fewer than minNeighbors
// neighbours, or all of them at one place) gets a zero normal and a NaN curvature.
func (k *KDTree) Normals(radius float32, viewpoint mat.Vec3, minNeighbors int) (normals []mat.Vec3, curvature []float32, counts []int32, err error) {
	return k.NormalsAt(nil, radius, viewpoint, minNeighbors)
}

// NormalsAt is Normals for arbitrary query points; q == nil takes the tree's own points.
func (k *KDTree) NormalsAt(q []mat.Vec3, radius float32, viewpoint mat.Vec3, minNeighbors int) ([]mat.Vec3, []float32, []int32, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var qp *C.float
	n := len(q)
	if q == nil {
		var ln C.int64_t
		if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
			return nil, nil, nil, err
		}
		n = int(ln)
	} else if n > 0 {
		qp = (*C.float)(unsafe.Pointer(&q[0]))
	}
	normals := make([]mat.Vec3, n)
	curvature := make([]float32, n)
	counts := make([]int32, n)
	if n == 0 {
		return normals, curvature, counts, nil
	}
	vp := viewpoint
	rc := C.pcgx_kdtree_normals(k.t.h, qp, C.int64_t(n), C.float(radius), (*C.float)(unsafe.Pointer(&vp[0])),
		C.int32_t(minNeighbors), (*C.float)(unsafe.Pointer(&normals[0])), (*C.float)(unsafe.Pointer(&curvature[0])),
		(*C.int32_t)(unsafe.Pointer(&counts[0])))
	runtime.KeepAlive(q)
	runtime.KeepAlive(normals)
	runtime.KeepAlive(curvature)
	runtime.KeepAlive(counts)
	if err := status(rc); err != nil {
		return nil, nil, nil, err
	}
	return normals, curvature, counts, nil
}

// MLS smooths the tree's own points by moving least squares (extension: no reference parity; include/pcgx.h,
// pcgx_kdtree_mls): every point is projected onto the plane (order 1) or the quadratic height field (order 2) fitted
// to its radius neighbourhood with Gauss weights of width sigma (<= 0: the radius).  The result is in the tree's id
// order.  kinds: 0 the point came back unchanged (normal zero), 1 projected onto the plane, 2 onto the polynomial.
func (k *KDTree) MLS(radius, sigma float32, order, minNeighbors int, viewpoint mat.Vec3) (points, normals []mat.Vec3, kinds, counts []int32, err error) {
	return k.MLSAt(nil, radius, sigma, order, minNeighbors, viewpoint)
}

// MLSAt is MLS for arbitrary query points; q == nil takes the tree's own points.
func (k *KDTree) MLSAt(q []mat.Vec3, radius, sigma float32, order, minNeighbors int, viewpoint mat.Vec3) ([]mat.Vec3, []mat.Vec3, []int32, []int32, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var qp *C.float
	n := len(q)
	if q == nil {
		var ln C.int64_t
		if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
			return nil, nil, nil, nil, err
		}
		n = int(ln)
	} else if n > 0 {
		qp = (*C.float)(unsafe.Pointer(&q[0]))
	}
	points := make([]mat.Vec3, n)
	normals := make([]mat.Vec3, n)
	kinds := make([]int32, n)
	counts := make([]int32, n)
	if n == 0 {
		return points, normals, kinds, counts, nil
	}
	if !(sigma > 0) {
		sigma = radius
	}
	vp := viewpoint
	rc := C.pcgx_kdtree_mls(k.t.h, qp, C.int64_t(n), C.float(radius), C.float(sigma), C.int32_t(order),
		C.int32_t(minNeighbors), (*C.float)(unsafe.Pointer(&vp[0])), (*C.float)(unsafe.Pointer(&points[0])),
		(*C.float)(unsafe.Pointer(&normals[0])), (*C.int32_t)(unsafe.Pointer(&kinds[0])),
		(*C.int32_t)(unsafe.Pointer(&counts[0])))
	runtime.KeepAlive(q)
	runtime.KeepAlive(points)
	runtime.KeepAlive(normals)
	runtime.KeepAlive(kinds)
	runtime.KeepAlive(counts)
	if err := status(rc); err != nil {
		return nil, nil, nil, nil, err
	}
	return points, normals, kinds, counts, nil
}

// FPFH returns the Fast Point Feature Histogram of every point of the tree over its radius neighbourhood (extension: no
// reference parity; include/pcgx.h, pcgx_kdtree_fpfh): 33 numbers per point in id order, eleven bins for each of the
// three pair features, each feature summing to 200 where the point has valid pairs.  normals: one per point in id
// order, e.g. what Normals returns; a zero normal takes its point out of every pair.
func (k *KDTree) FPFH(radius float32, normals []mat.Vec3) ([][33]float32, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, err
	}
	n := int(ln)
	if len(normals) != n {
		return nil, errors.New("pcgx: one normal per point of the tree is required")
	}
	fpfh := make([][33]float32, n)
	if n == 0 {
		return fpfh, nil
	}
	rc := C.pcgx_kdtree_fpfh(k.t.h, (*C.float)(unsafe.Pointer(&normals[0])), C.float(radius),
		(*C.float)(unsafe.Pointer(&fpfh[0])), nil, nil)
	runtime.KeepAlive(normals)
	runtime.KeepAlive(fpfh)
	if err := status(rc); err != nil {
		return nil, err
	}
	return fpfh, nil
}

// FPFHAt returns FPFH's rows at the listed point ids only, and the points themselves (extension: no reference parity;
// include/pcgx.h, pcgx_kdtree_fpfh_at): row s is FPFH(radius, normals)'s row ids[s] bit for bit, without describing the
// rest of the cloud.  ids: in any order, repeats allowed, e.g. what ISSKeypoints returns; an id outside [0, Len()) is
// an error.  nSpfh: how many points' SPFH records had to be computed, the listed points and their neighbours.
func (k *KDTree) FPFHAt(radius float32, normals []mat.Vec3, ids []int) (fpfh [][33]float32, xyz []mat.Vec3, nSpfh int, err error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, nil, 0, err
	}
	if len(normals) != int(ln) {
		return nil, nil, 0, errors.New("pcgx: one normal per point of the tree is required")
	}
	fpfh = make([][33]float32, len(ids))
	xyz = make([]mat.Vec3, len(ids))
	if len(ids) == 0 {
		return fpfh, xyz, 0, nil
	}
	ids64 := make([]C.int64_t, len(ids))
	for i, id := range ids {
		ids64[i] = C.int64_t(id)
	}
	var np *C.float // (an empty tree: every id is out of range, and the library says so)
	if len(normals) > 0 {
		np = (*C.float)(unsafe.Pointer(&normals[0]))
	}
	var cnt C.int64_t
	rc := C.pcgx_kdtree_fpfh_at(k.t.h, np, C.float(radius), &ids64[0], C.int64_t(len(ids)),
		(*C.float)(unsafe.Pointer(&fpfh[0])), (*C.float)(unsafe.Pointer(&xyz[0])), nil, nil, &cnt)
	runtime.KeepAlive(normals)
	runtime.KeepAlive(ids64)
	runtime.KeepAlive(fpfh)
	runtime.KeepAlive(xyz)
	if err := status(rc); err != nil {
		return nil, nil, 0, err
	}
	return fpfh, xyz, int(cnt), nil
}

// LocalMaxima returns, in ascending order, the ids of the points whose score is the largest of their radius
// neighbourhood (extension: no reference parity; include/pcgx.h, pcgx_kdtree_local_maxima).  score: one per point in id
// order; only a score > 0 qualifies (NaN never, +Inf does), ties go to the smaller id, a deleted id is never a maximum.
func (k *KDTree) LocalMaxima(radius float32, score []float32) ([]int64, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, err
	}
	n := int(ln)
	if len(score) != n {
		return nil, errors.New("pcgx: one score per point of the tree is required")
	}
	ids := make([]int64, n)
	if n == 0 {
		return ids, nil
	}
	var m C.int64_t
	rc := C.pcgx_kdtree_local_maxima(k.t.h, C.float(radius), (*C.float)(unsafe.Pointer(&score[0])),
		(*C.int64_t)(unsafe.Pointer(&ids[0])), &m)
	runtime.KeepAlive(score)
	runtime.KeepAlive(ids)
	if err := status(rc); err != nil {
		return nil, err
	}
	return ids[:int(m)], nil
}

// Thin returns a maximal subset of the tree's own points no two of which are within radius of each other, ascending ids,
// and per point in id order the kept point that stands for it (extension: no reference parity; include/pcgx.h,
// pcgx_kdtree_thin).  The set is what greedy selection in priority order keeps: by hash(seed, id) where score is nil,
// else the larger score first, ties to the smaller id.  owner: a kept point itself, a dropped point its kept neighbour
// of the smallest (DistSq, id), -1 for a deleted id, a non-finite point or a NaN score.
func (k *KDTree) Thin(radius float32, seed uint32, score []float32) (ids, owner []int64, err error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, nil, err
	}
	n := int(ln)
	if score != nil && len(score) != n {
		return nil, nil, errors.New("pcgx: one score per point of the tree is required")
	}
	ids = make([]int64, n)
	owner = make([]int64, n)
	if n == 0 {
		return ids, owner, nil
	}
	var sp *C.float
	if score != nil {
		sp = (*C.float)(unsafe.Pointer(&score[0]))
	}
	var m C.int64_t
	rc := C.pcgx_kdtree_thin(k.t.h, C.float(radius), C.uint32_t(seed), sp, (*C.int64_t)(unsafe.Pointer(&ids[0])), &m,
		(*C.int64_t)(unsafe.Pointer(&owner[0])))
	runtime.KeepAlive(score)
	runtime.KeepAlive(ids)
	runtime.KeepAlive(owner)
	if err := status(rc); err != nil {
		return nil, nil, err
	}
	return ids[:int(m)], owner, nil
}

// FarthestResult is what (*KDTree).FarthestPoints returns: the picks in pick order, the d of each pick at the moment it
// was picked (the first +Inf, then non-increasing), the d the next pick would have had (-1 when no point is left), and
// per point in id order the id of the pick nearest to it (the earlier pick among equal distances, -1 for a deleted id or
// a non-finite point).
type FarthestResult struct {
	IDs     []int64
	DistSq  []float32
	CoverSq float32
	Owner   []int64
}

// FarthestPoints returns count of the tree's own points, each the one farthest from those picked before it (float32
// DistSq to the nearest pick so far, ties to the smallest id), starting at start or, for -1, at the smallest eligible id
// (extension: no reference parity; include/pcgx.h, pcgx_kdtree_fps).  There are min(count, eligible points) picks, and
// they are the first picks of any larger count: one call orders a cloud so that every prefix is a sampling of its own.
func (k *KDTree) FarthestPoints(count int, start int64) (*FarthestResult, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	if count < 0 {
		return nil, errors.New("pcgx: count must be >= 0")
	}
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, err
	}
	n := int(ln)
	res := &FarthestResult{IDs: make([]int64, count), DistSq: make([]float32, count), CoverSq: -1, Owner: make([]int64, n)}
	var ip, op *C.int64_t
	var dp *C.float
	if count > 0 {
		ip = (*C.int64_t)(unsafe.Pointer(&res.IDs[0]))
		dp = (*C.float)(unsafe.Pointer(&res.DistSq[0]))
	}
	if n > 0 {
		op = (*C.int64_t)(unsafe.Pointer(&res.Owner[0]))
	}
	var m C.int64_t
	var cover C.float
	rc := C.pcgx_kdtree_fps(k.t.h, C.int64_t(count), C.int64_t(start), ip, &m, dp, &cover, op)
	runtime.KeepAlive(res)
	if err := status(rc); err != nil {
		return nil, err
	}
	res.IDs, res.DistSq, res.CoverSq = res.IDs[:int(m)], res.DistSq[:int(m)], float32(cover)
	return res, nil
}

// OrientMode says how (*KDTree).OrientNormals fixes the overall sign of a component: OrientKeep leaves its smallest id
// as given, OrientDirection makes its topmost point along ref look along ref (Hoppe's rule), OrientViewpoint makes the
// majority of its normals look towards ref.
type OrientMode int32

const (
	OrientKeep      OrientMode = 0
	OrientDirection OrientMode = 1
	OrientViewpoint OrientMode = 2
)

// OrientedNormals is what (*KDTree).OrientNormals returns, everything in id order: the normals (3 floats per point, the
// given bits with the signs inverted where Flipped), the flags, the smallest id of each point's component (-1 for a
// point that takes no part: a deleted id, a non-finite point, a zero or non-finite normal), and the component count.
type OrientedNormals struct {
	Normals    []float32
	Flipped    []uint8
	Component  []int64
	Components int64
}

// OrientNormals gives neighbouring normals (DistSq < radius^2, Range's set) the same side: the sign is carried along the
// minimum spanning forest of the radius graph, its edges ordered by |n_i . n_j| descending, then the smaller ids
// (extension: no reference parity; include/pcgx.h, pcgx_kdtree_orient_normals).  normals: 3 floats per point in id order.
func (k *KDTree) OrientNormals(radius float32, normals []float32, mode OrientMode, ref [3]float32) (*OrientedNormals, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, err
	}
	n := int(ln)
	if len(normals) != 3*n {
		return nil, errors.New("pcgx: one normal per point of the tree is required")
	}
	res := &OrientedNormals{Normals: make([]float32, 3*n), Flipped: make([]uint8, n), Component: make([]int64, n)}
	var np, op *C.float
	var fp *C.uint8_t
	var cp *C.int64_t
	if n > 0 {
		np = (*C.float)(unsafe.Pointer(&normals[0]))
		op = (*C.float)(unsafe.Pointer(&res.Normals[0]))
		fp = (*C.uint8_t)(unsafe.Pointer(&res.Flipped[0]))
		cp = (*C.int64_t)(unsafe.Pointer(&res.Component[0]))
	}
	var nc, open C.int64_t
	rc := C.pcgx_kdtree_orient_normals(k.t.h, C.float(radius), np, C.int32_t(mode), (*C.float)(unsafe.Pointer(&ref[0])), op,
		fp, cp, &nc, &open)
	runtime.KeepAlive(normals)
	runtime.KeepAlive(res)
	if err := status(rc); err != nil {
		return nil, err
	}
	res.Components = int64(nc)
	return res, nil
}

// BoundaryPoints is what (*KDTree).Boundary returns: the boundary points' ids ascending, and per point in id order the
// longest cyclic run of empty sectors (64 for an empty mask, -1 where the point is not evaluated), the mask of the
// sectors a neighbour falls in, and the neighbourhood's size.
type BoundaryPoints struct {
	IDs    []int64
	Gaps   []int32
	Masks  []uint64
	Counts []int32
}

// Boundary returns the points whose radius neighbours leave an angular gap of at least minGap sectors of 5.625 degrees
// (1..64; 16 is PCL's pi / 2) in the tangent plane of normals, one per point in id order (extension: no reference
// parity; include/pcgx.h, pcgx_kdtree_boundary).  A true opening of g sectors gives g - 2 < gap < g.
func (k *KDTree) Boundary(radius float32, normals []mat.Vec3, minGap, minNeighbors int) (*BoundaryPoints, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, err
	}
	n := int(ln)
	if len(normals) != n {
		return nil, errors.New("pcgx: one normal per point of the tree is required")
	}
	res := &BoundaryPoints{IDs: make([]int64, n), Gaps: make([]int32, n), Masks: make([]uint64, n), Counts: make([]int32, n)}
	if n == 0 {
		return res, nil
	}
	var m C.int64_t
	rc := C.pcgx_kdtree_boundary(k.t.h, C.float(radius), (*C.float)(unsafe.Pointer(&normals[0])), C.int32_t(minGap),
		C.int32_t(minNeighbors), (*C.int64_t)(unsafe.Pointer(&res.IDs[0])), &m, (*C.int32_t)(unsafe.Pointer(&res.Gaps[0])),
		(*C.uint64_t)(unsafe.Pointer(&res.Masks[0])), (*C.int32_t)(unsafe.Pointer(&res.Counts[0])))
	runtime.KeepAlive(normals)
	runtime.KeepAlive(res)
	if err := status(rc); err != nil {
		return nil, err
	}
	res.IDs = res.IDs[:int(m)]
	return res, nil
}

// RayHits is what (*KDTree).RayCast returns, per ray: the first point's id (-1: none), Along = (p - o) . d and
// OffSq = |(p - o) x d|^2 in float64 (0 for a miss).
type RayHits struct {
	IDs   []int64
	Along []float64
	OffSq []float64
}

// rayArgs checks one direction (and one sMin, sMax where given) per origin and returns the C pointers (nil: absent).
func rayArgs(origins, directions []mat.Vec3, sMin, sMax []float32) (o, d, lo, hi *C.float, err error) {
	nr := len(origins)
	if len(directions) != nr || (sMin != nil && len(sMin) != nr) || (sMax != nil && len(sMax) != nr) {
		return nil, nil, nil, nil, errors.New("pcgx: one direction (and one sMin, sMax where given) per origin is required")
	}
	if nr > 0 {
		o, d = (*C.float)(unsafe.Pointer(&origins[0])), (*C.float)(unsafe.Pointer(&directions[0]))
		if sMin != nil {
			lo = (*C.float)(unsafe.Pointer(&sMin[0]))
		}
		if sMax != nil {
			hi = (*C.float)(unsafe.Pointer(&sMax[0]))
		}
	}
	return o, d, lo, hi, nil
}

// RayCast returns, for each ray origins[j] + s directions[j] with s in [sMin[j], sMax[j]] (nil: 0 and +inf), the first
// of the tree's points within radius of the ray's line: the member with the smallest Along, a tie going to the smallest
// id.  Directions are not normalised: s = Along / |d|^2 (extension: no reference parity; include/pcgx.h,
// pcgx_kdtree_raycast).
func (k *KDTree) RayCast(origins, directions []mat.Vec3, radius float32, sMin, sMax []float32) (*RayHits, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	o, d, lo, hi, err := rayArgs(origins, directions, sMin, sMax)
	if err != nil {
		return nil, err
	}
	nr := len(origins)
	res := &RayHits{IDs: make([]int64, nr), Along: make([]float64, nr), OffSq: make([]float64, nr)}
	if nr == 0 {
		return res, nil
	}
	rc := C.pcgx_kdtree_raycast(k.t.h, o, d, lo, hi, C.int64_t(nr), C.float(radius), (*C.int64_t)(unsafe.Pointer(&res.IDs[0])),
		(*C.double)(unsafe.Pointer(&res.Along[0])), (*C.double)(unsafe.Pointer(&res.OffSq[0])))
	runtime.KeepAlive(origins)
	runtime.KeepAlive(directions)
	runtime.KeepAlive(sMin)
	runtime.KeepAlive(sMax)
	runtime.KeepAlive(res)
	if err := status(rc); err != nil {
		return nil, err
	}
	return res, nil
}

// RayPierce returns, per point in id order, how many of the rays it lies in the tube of (RayCast's member test; a
// deleted point counts 0): what free-space carving asks of a map (extension: no reference parity; include/pcgx.h,
// pcgx_kdtree_ray_pierce).
func (k *KDTree) RayPierce(origins, directions []mat.Vec3, radius float32, sMin, sMax []float32) ([]int32, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	o, d, lo, hi, err := rayArgs(origins, directions, sMin, sMax)
	if err != nil {
		return nil, err
	}
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, err
	}
	counts := make([]int32, int(ln))
	if len(counts) == 0 || len(origins) == 0 {
		return counts, nil
	}
	rc := C.pcgx_kdtree_ray_pierce(k.t.h, o, d, lo, hi, C.int64_t(len(origins)), C.float(radius),
		(*C.int32_t)(unsafe.Pointer(&counts[0])))
	runtime.KeepAlive(origins)
	runtime.KeepAlive(directions)
	runtime.KeepAlive(sMin)
	runtime.KeepAlive(sMax)
	if err := status(rc); err != nil {
		return nil, err
	}
	return counts, nil
}

// CylinderStats is what (*KDTree).CylinderStats returns, per cylinder: the number of the tree's live points in it and,
// at Sums[2j] and Sums[2j+1], S1 = the sum of a and S2 = the sum of a a, a = (p - core) . axis in float64,
// unnormalised.
type CylinderStats struct {
	Counts []int32
	Sums   []float64
}

// CylinderStats returns the statistics of the cylinders with cores[j], axes[j] (not normalised), radius and halfLength
// each way along the axis, over the tree's live points: what M3C2Finish turns into distances (extension: no reference
// parity; include/pcgx.h, pcgx_kdtree_cylinder_stats).
func (k *KDTree) CylinderStats(cores, axes []mat.Vec3, radius, halfLength float32) (*CylinderStats, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	m := len(cores)
	if len(axes) != m {
		return nil, errors.New("pcgx: one axis per core is required")
	}
	res := &CylinderStats{Counts: make([]int32, m), Sums: make([]float64, 2*m)}
	if m == 0 {
		return res, nil
	}
	rc := C.pcgx_kdtree_cylinder_stats(k.t.h, (*C.float)(unsafe.Pointer(&cores[0])), (*C.float)(unsafe.Pointer(&axes[0])),
		C.int64_t(m), C.float(radius), C.float(halfLength), (*C.int32_t)(unsafe.Pointer(&res.Counts[0])),
		(*C.double)(unsafe.Pointer(&res.Sums[0])))
	runtime.KeepAlive(cores)
	runtime.KeepAlive(axes)
	runtime.KeepAlive(res)
	if err := status(rc); err != nil {
		return nil, err
	}
	return res, nil
}

// M3C2Result is what M3C2Finish returns, per core: the signed distance along the axis, epoch 2 minus epoch 1, the level
// of detection at 95 % and whether |Distance| exceeds it (NaN, NaN, false where a cylinder held too few points or the
// axis is unusable).
type M3C2Result struct {
	Distance    []float64
	LoD         []float64
	Significant []bool
}

// M3C2Finish is M3C2's finish (Lague, Brodu and Leroux 2013) on the cylinder statistics of two epochs, taken with the
// same cores, axes, radius and half length against each epoch's tree (extension: no reference parity; include/pcgx.h,
// pcgx_m3c2_finish).
func M3C2Finish(axes []mat.Vec3, epoch1, epoch2 *CylinderStats, registrationError float64, minCount int32) (*M3C2Result, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	m := len(axes)
	if epoch1 == nil || epoch2 == nil || len(epoch1.Counts) != m || len(epoch2.Counts) != m || len(epoch1.Sums) != 2*m ||
		len(epoch2.Sums) != 2*m {
		return nil, errors.New("pcgx: one count and two sums per axis and epoch are required")
	}
	res := &M3C2Result{Distance: make([]float64, m), LoD: make([]float64, m), Significant: make([]bool, m)}
	if m == 0 {
		return res, nil
	}
	sig := make([]uint8, m)
	rc := C.pcgx_m3c2_finish((*C.float)(unsafe.Pointer(&axes[0])), (*C.int32_t)(unsafe.Pointer(&epoch1.Counts[0])),
		(*C.double)(unsafe.Pointer(&epoch1.Sums[0])), (*C.int32_t)(unsafe.Pointer(&epoch2.Counts[0])),
		(*C.double)(unsafe.Pointer(&epoch2.Sums[0])), C.int64_t(m), C.double(registrationError), C.int32_t(minCount),
		(*C.double)(unsafe.Pointer(&res.Distance[0])), (*C.double)(unsafe.Pointer(&res.LoD[0])),
		(*C.uint8_t)(unsafe.Pointer(&sig[0])))
	runtime.KeepAlive(axes)
	runtime.KeepAlive(epoch1)
	runtime.KeepAlive(epoch2)
	runtime.KeepAlive(res)
	if err := status(rc); err != nil {
		return nil, err
	}
	for i, v := range sig {
		res.Significant[i] = v != 0
	}
	return res, nil
}

// ISSKeypoints returns the ISS keypoints of the tree's points (Zhong 2009, Open3D's form; extension: no reference
// parity; include/pcgx.h, pcgx_kdtree_iss_keypoints): ids ascending, and per point in id order the eigenvalues of
// Normals' covariance at salientRadius (ascending, zero where Normals answers "degenerate") and the saliency (the
// smallest eigenvalue where l1 < gamma21 l2 and l0 < gamma32 l1, else 0).  The keypoints are LocalMaxima(nonMaxRadius,
// saliency).  The usual parameters: gamma21 = gamma32 = 0.975, minNeighbors = 5.
func (k *KDTree) ISSKeypoints(salientRadius, nonMaxRadius, gamma21, gamma32 float32, minNeighbors int) (ids []int64, eigenvalues []mat.Vec3, saliency []float32, err error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, nil, nil, err
	}
	n := int(ln)
	ids = make([]int64, n)
	eigenvalues = make([]mat.Vec3, n)
	saliency = make([]float32, n)
	if n == 0 {
		return ids, eigenvalues, saliency, nil
	}
	var m C.int64_t
	rc := C.pcgx_kdtree_iss_keypoints(k.t.h, C.float(salientRadius), C.float(nonMaxRadius), C.float(gamma21),
		C.float(gamma32), C.int32_t(minNeighbors), (*C.float)(unsafe.Pointer(&eigenvalues[0])),
		(*C.float)(unsafe.Pointer(&saliency[0])), (*C.int64_t)(unsafe.Pointer(&ids[0])), &m)
	runtime.KeepAlive(ids)
	runtime.KeepAlive(eigenvalues)
	runtime.KeepAlive(saliency)
	if err := status(rc); err != nil {
		return nil, nil, nil, err
	}
	return ids[:int(m)], eigenvalues, saliency, nil
}

// ClusterParams are the optional parts of (*KDTree).Clusters.  Normals (nil: none): an edge also needs
// |n_i . n_j| >= MinCos (n_i . n_j when Oriented), and a point whose normal is not finite or zero belongs to no
// cluster.  Curvature (nil: none): a point above MaxCurvature, or NaN, belongs to no cluster.  A cluster has
// max(MinSize, 1) <= size, and size <= MaxSize unless MaxSize is 0.
type ClusterParams struct {
	Normals      []mat.Vec3
	MinCos       float32
	Oriented     bool
	Curvature    []float32
	MaxCurvature float32
	MinSize      int64
	MaxSize      int64
}

// Clusters returns the connected components of the radius graph over the tree's points (extension: no reference
// parity; include/pcgx.h, pcgx_kdtree_clusters), largest first, equal sizes by smallest id: labels per point in id
// order (the cluster's number, or -1), sizes per cluster, and ids: the members of cluster 0 ascending, then those of
// cluster 1, and so on (cluster c starts at the sum of the sizes before it).
func (k *KDTree) Clusters(radius float32, p ClusterParams) (labels, sizes, ids []int64, err error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, nil, nil, err
	}
	n := int(ln)
	if p.Normals != nil && len(p.Normals) != n {
		return nil, nil, nil, errors.New("pcgx: one normal per point of the tree is required")
	}
	if p.Curvature != nil && len(p.Curvature) != n {
		return nil, nil, nil, errors.New("pcgx: one curvature per point of the tree is required")
	}
	labels = make([]int64, n)
	sizes = make([]int64, n)
	ids = make([]int64, n)
	if n == 0 {
		return labels, sizes, ids, nil
	}
	var nrm, cur *C.float
	if p.Normals != nil {
		nrm = (*C.float)(unsafe.Pointer(&p.Normals[0]))
	}
	if p.Curvature != nil {
		cur = (*C.float)(unsafe.Pointer(&p.Curvature[0]))
	}
	oriented := C.int32_t(0)
	if p.Oriented {
		oriented = 1
	}
	var c C.int64_t
	rc := C.pcgx_kdtree_clusters(k.t.h, C.float(radius), nrm, C.float(p.MinCos), oriented, cur, C.float(p.MaxCurvature),
		C.int64_t(p.MinSize), C.int64_t(p.MaxSize), (*C.int64_t)(unsafe.Pointer(&labels[0])), &c,
		(*C.int64_t)(unsafe.Pointer(&sizes[0])), (*C.int64_t)(unsafe.Pointer(&ids[0])))
	runtime.KeepAlive(p.Normals)
	runtime.KeepAlive(p.Curvature)
	runtime.KeepAlive(labels)
	runtime.KeepAlive(sizes)
	runtime.KeepAlive(ids)
	if err := status(rc); err != nil {
		return nil, nil, nil, err
	}
	sizes = sizes[:int(c)]
	total := int64(0)
	for _, s := range sizes {
		total += s
	}
	return labels, sizes, ids[:int(total)], nil
}

// DBSCAN returns the density clusters of the tree's points (extension: no reference parity; include/pcgx.h,
// pcgx_kdtree_dbscan): a point with at least minPts points within radius (DistSq < radius^2, itself included) is
// core; a cluster is a component of core points plus its border points, each with its nearest core neighbour
// (smallest DistSq, then smallest id); kept when max(minSize, 1) <= size, and size <= maxSize unless maxSize is 0.
// labels, sizes and ids as Clusters returns them; kind per point: 0 noise, 1 border, 2 core.
func (k *KDTree) DBSCAN(radius float32, minPts int32, minSize, maxSize int64) (labels, sizes, ids []int64, kind []uint8, err error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, nil, nil, nil, err
	}
	n := int(ln)
	labels = make([]int64, n)
	sizes = make([]int64, n)
	ids = make([]int64, n)
	kind = make([]uint8, n)
	if n == 0 {
		return labels, sizes, ids, kind, nil
	}
	var c C.int64_t
	rc := C.pcgx_kdtree_dbscan(k.t.h, C.float(radius), C.int32_t(minPts), C.int64_t(minSize), C.int64_t(maxSize),
		(*C.int64_t)(unsafe.Pointer(&labels[0])), &c, (*C.int64_t)(unsafe.Pointer(&sizes[0])),
		(*C.int64_t)(unsafe.Pointer(&ids[0])), (*C.uint8_t)(unsafe.Pointer(&kind[0])))
	runtime.KeepAlive(labels)
	runtime.KeepAlive(sizes)
	runtime.KeepAlive(ids)
	runtime.KeepAlive(kind)
	if err := status(rc); err != nil {
		return nil, nil, nil, nil, err
	}
	sizes = sizes[:int(c)]
	total := int64(0)
	for _, s := range sizes {
		total += s
	}
	return labels, sizes, ids[:int(total)], kind, nil
}

// PlanesParams are the options of (*KDTree).Planes: NHyp hypotheses a round and at most MaxPlanes rounds; a round's best
// needs max(MinInliers, 3) inliers; Axis (nil: none): only planes whose normal has |cos| >= MinAxisCos with it; Normals
// (nil: none; 3 per point): an inlier's normal has |cos| >= MinNormalCos with the plane's; Refine: one least-squares
// refit of the best to its inliers, kept where it loses no inlier.
type PlanesParams struct {
	NHyp         int64
	MaxPlanes    int32
	MinInliers   int64
	Axis         *[3]float32
	MinAxisCos   float32
	Normals      []float32
	MinNormalCos float32
	Refine       bool
}

// PlaneSegments is the result of (*KDTree).Planes: Planes holds (nx, ny, nz, d) per plane found, Sizes, Refined and Best
// one entry per plane, Labels per point the plane that took it or -1, IDs the inliers plane by plane (ascending inside
// a plane): Sizes and IDs are a grouped list for GroupStats and GroupHulls.
type PlaneSegments struct {
	Planes  []float32
	Sizes   []int64
	Refined []int32
	Best    []int64
	Labels  []int64
	IDs     []int64
}

// Planes segments the tree's live points into planes (extension: no reference parity; include/pcgx.h,
// pcgx_kdtree_planes): the plane most points lie within maxDist of, by sample consensus over the caller's random words
// (samples: 3 per hypothesis and round, 3 * NHyp * MaxPlanes in all), its inliers taken out, then the next.
func (k *KDTree) Planes(maxDist float32, samples []uint32, p PlanesParams) (*PlaneSegments, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, err
	}
	n := int(ln)
	if p.Normals != nil && len(p.Normals) != 3*n {
		return nil, errors.New("pcgx: one normal per point of the tree is required")
	}
	if p.NHyp > 0 && p.MaxPlanes > 0 && int64(len(samples)) != 3*p.NHyp*int64(p.MaxPlanes) {
		return nil, errors.New("pcgx: three sample words per hypothesis and round are required")
	}
	mp := int(p.MaxPlanes)
	if mp < 1 {
		mp = 1 // (the call refuses MaxPlanes < 1; the outputs must exist all the same)
	}
	r := &PlaneSegments{Planes: make([]float32, 4*mp), Sizes: make([]int64, mp), Refined: make([]int32, mp),
		Best: make([]int64, mp), Labels: make([]int64, n+1), IDs: make([]int64, n+1)}
	var smp *C.uint32_t
	if len(samples) > 0 {
		smp = (*C.uint32_t)(unsafe.Pointer(&samples[0]))
	}
	var axis, nrm *C.float
	if p.Axis != nil {
		axis = (*C.float)(unsafe.Pointer(&p.Axis[0]))
	}
	if len(p.Normals) > 0 {
		nrm = (*C.float)(unsafe.Pointer(&p.Normals[0]))
	}
	refine := C.int32_t(0)
	if p.Refine {
		refine = 1
	}
	var c C.int64_t
	rc := C.pcgx_kdtree_planes(k.t.h, smp, C.int64_t(p.NHyp), C.int32_t(p.MaxPlanes), C.float(maxDist), C.int64_t(p.MinInliers),
		axis, C.float(p.MinAxisCos), nrm, C.float(p.MinNormalCos), refine, &c, (*C.float)(unsafe.Pointer(&r.Planes[0])),
		(*C.int64_t)(unsafe.Pointer(&r.Sizes[0])), (*C.int32_t)(unsafe.Pointer(&r.Refined[0])),
		(*C.int64_t)(unsafe.Pointer(&r.Best[0])), (*C.int64_t)(unsafe.Pointer(&r.Labels[0])),
		(*C.int64_t)(unsafe.Pointer(&r.IDs[0])), nil, nil, nil)
	runtime.KeepAlive(samples)
	runtime.KeepAlive(p.Normals)
	runtime.KeepAlive(p.Axis)
	runtime.KeepAlive(r)
	if err := status(rc); err != nil {
		return nil, err
	}
	found := int(c)
	total := int64(0)
	for _, s := range r.Sizes[:found] {
		total += s
	}
	r.Planes, r.Sizes, r.Refined, r.Best = r.Planes[:4*found], r.Sizes[:found], r.Refined[:found], r.Best[:found]
	r.Labels, r.IDs = r.Labels[:n], r.IDs[:int(total)]
	return r, nil
}

// The kinds of shape (*KDTree).Shapes looks for.
const (
	ShapeSphere   int32 = 0
	ShapeCylinder int32 = 1
)

// ShapesParams are the options of (*KDTree).Shapes: NHyp hypotheses a round and at most MaxShapes rounds; a round's best
// needs max(MinInliers, 2) inliers; SampleRadius: a hypothesis's second point comes out of this radius about its first
// (0: out of everything left); RMin <= r <= RMax (RMax 0 stands for no upper limit); Axis (nil: none): only cylinders
// whose axis has |cos| >= MinAxisCos with it; an inlier's normal has |cos| >= MinNormalCos with the shape's; Refine: one
// least-squares refit of the best's centre and radius to its inliers, kept where it loses no inlier.
type ShapesParams struct {
	NHyp         int64
	MaxShapes    int32
	MinInliers   int64
	SampleRadius float32
	RMin, RMax   float32
	Axis         *[3]float32
	MinAxisCos   float32
	MinNormalCos float32
	Refine       bool
}

// ShapeSegments is the result of (*KDTree).Shapes: Shapes holds 8 numbers per shape found, (cx, cy, cz, r, 0, 0, 0, 0)
// for a sphere and (qx, qy, qz, r, ax, ay, az, 0) for a cylinder (q the axis point nearest the origin); Sizes, Refined
// and Best one entry per shape, Labels per point the shape that took it or -1, IDs the inliers shape by shape (ascending
// inside a shape): Sizes and IDs are a grouped list for GroupStats and GroupHulls.
type ShapeSegments struct {
	Shapes  []float32
	Sizes   []int64
	Refined []int32
	Best    []int64
	Labels  []int64
	IDs     []int64
}

// Shapes segments the tree's live points into spheres or cylinders (extension: no reference parity; include/pcgx.h,
// pcgx_kdtree_shapes): the shape most points lie within maxDist of, by sample consensus over hypotheses made from two
// oriented points drawn by the caller's random words (samples: 2 per hypothesis and round, 2 * NHyp * MaxShapes in all),
// its inliers taken out, then the next.  normals: 3 per point of the tree.
func (k *KDTree) Shapes(kind int32, maxDist float32, normals []float32, samples []uint32, p ShapesParams) (*ShapeSegments, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, err
	}
	n := int(ln)
	if len(normals) != 3*n {
		return nil, errors.New("pcgx: one normal per point of the tree is required")
	}
	if p.NHyp > 0 && p.MaxShapes > 0 && int64(len(samples)) != 2*p.NHyp*int64(p.MaxShapes) {
		return nil, errors.New("pcgx: two sample words per hypothesis and round are required")
	}
	mp := int(p.MaxShapes)
	if mp < 1 {
		mp = 1 // (the call refuses MaxShapes < 1; the outputs must exist all the same)
	}
	r := &ShapeSegments{Shapes: make([]float32, 8*mp), Sizes: make([]int64, mp), Refined: make([]int32, mp),
		Best: make([]int64, mp), Labels: make([]int64, n+1), IDs: make([]int64, n+1)}
	var smp *C.uint32_t
	if len(samples) > 0 {
		smp = (*C.uint32_t)(unsafe.Pointer(&samples[0]))
	}
	var axis, nrm *C.float
	if p.Axis != nil {
		axis = (*C.float)(unsafe.Pointer(&p.Axis[0]))
	}
	if len(normals) > 0 {
		nrm = (*C.float)(unsafe.Pointer(&normals[0]))
	}
	refine := C.int32_t(0)
	if p.Refine {
		refine = 1
	}
	rMax := p.RMax
	if rMax == 0 {
		rMax = float32(math.Inf(1))
	}
	var c C.int64_t
	rc := C.pcgx_kdtree_shapes(k.t.h, C.int32_t(kind), smp, C.int64_t(p.NHyp), C.int32_t(p.MaxShapes), C.float(maxDist),
		C.int64_t(p.MinInliers), C.float(p.SampleRadius), C.float(p.RMin), C.float(rMax), axis, C.float(p.MinAxisCos), nrm,
		C.float(p.MinNormalCos), refine, &c, (*C.float)(unsafe.Pointer(&r.Shapes[0])),
		(*C.int64_t)(unsafe.Pointer(&r.Sizes[0])), (*C.int32_t)(unsafe.Pointer(&r.Refined[0])),
		(*C.int64_t)(unsafe.Pointer(&r.Best[0])), (*C.int64_t)(unsafe.Pointer(&r.Labels[0])),
		(*C.int64_t)(unsafe.Pointer(&r.IDs[0])), nil, nil, nil)
	runtime.KeepAlive(samples)
	runtime.KeepAlive(normals)
	runtime.KeepAlive(p.Axis)
	runtime.KeepAlive(r)
	if err := status(rc); err != nil {
		return nil, err
	}
	found := int(c)
	total := int64(0)
	for _, s := range r.Sizes[:found] {
		total += s
	}
	r.Shapes, r.Sizes, r.Refined, r.Best = r.Shapes[:8*found], r.Sizes[:found], r.Refined[:found], r.Best[:found]
	r.Labels, r.IDs = r.Labels[:n], r.IDs[:int(total)]
	return r, nil
}

// GroundGrid is the grid (*KDTree).Ground works on: its corner (x, y), its size in cells (nx, ny) and the cell's side.
type GroundGrid struct {
	Origin [2]float32
	Dims   [2]int32
	Cell   float32
}

// GroundSegments is the result of (*KDTree).Ground: Labels per point (0 ground, 1 not ground, -1 no part), Sizes of the
// two groups, IDs the ground ascending, then the rest (a grouped list for GroupStats and GroupHulls), Window the first
// window a point failed (-1: ground), Surface the terrain model (Dims[1] rows of Dims[0], +Inf at an empty cell) and HAG
// the height above it per point (NaN where the point takes no part).
type GroundSegments struct {
	Labels  []int64
	Sizes   []int64
	IDs     []int64
	Window  []int32
	Surface []float32
	HAG     []float32
}

// Ground segments the tree's live points into ground and the rest by a progressive morphological filter (extension: no
// reference parity; include/pcgx.h, pcgx_kdtree_ground): the minimum z surface over the grid is opened with squares of
// half[k] cells one after the other, and a point is ground iff z - surface_k < height[k] after every window k.
func (k *KDTree) Ground(g GroundGrid, half []int32, height []float32) (*GroundSegments, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var ln C.int64_t
	if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
		return nil, err
	}
	n := int(ln)
	if len(half) != len(height) {
		return nil, errors.New("pcgx: one height per window is required")
	}
	cells := 1
	if g.Dims[0] >= 1 && g.Dims[0] <= 8192 && g.Dims[1] >= 1 && g.Dims[1] <= 8192 {
		cells = int(g.Dims[0]) * int(g.Dims[1]) // (the call refuses other sizes; the output must exist all the same)
	}
	r := &GroundSegments{Labels: make([]int64, n+1), Sizes: make([]int64, 2), IDs: make([]int64, n+1),
		Window: make([]int32, n+1), Surface: make([]float32, cells), HAG: make([]float32, n+1)}
	var hf *C.int32_t
	var ht *C.float
	if len(half) > 0 {
		hf = (*C.int32_t)(unsafe.Pointer(&half[0]))
		ht = (*C.float)(unsafe.Pointer(&height[0]))
	}
	var c C.int64_t
	rc := C.pcgx_kdtree_ground(k.t.h, (*C.float)(unsafe.Pointer(&g.Origin[0])), (*C.int32_t)(unsafe.Pointer(&g.Dims[0])),
		C.float(g.Cell), C.int32_t(len(half)), hf, ht, (*C.int64_t)(unsafe.Pointer(&r.Labels[0])),
		(*C.int64_t)(unsafe.Pointer(&r.Sizes[0])), (*C.int64_t)(unsafe.Pointer(&r.IDs[0])), &c,
		(*C.int32_t)(unsafe.Pointer(&r.Window[0])), (*C.float)(unsafe.Pointer(&r.Surface[0])),
		(*C.float)(unsafe.Pointer(&r.HAG[0])))
	runtime.KeepAlive(half)
	runtime.KeepAlive(height)
	runtime.KeepAlive(r)
	if err := status(rc); err != nil {
		return nil, err
	}
	r.Labels, r.IDs = r.Labels[:n], r.IDs[:int(r.Sizes[0]+r.Sizes[1])]
	r.Window, r.HAG = r.Window[:n], r.HAG[:n]
	return r, nil
}

// GroupGeometry is the result of (*KDTree).GroupStats, one row per group: Count of live members; AABB lo x, y, z then
// hi x, y, z; Centroid; Cov in the order xx, xy, xz, yy, yz, zz; Eig descending; Axes: the three unit eigenvectors as
// rows (axis 2 is the fitted plane's normal); OBB: centre x, y, z, then the half-extents along the axes.  A group
// without a live member is all zero.
type GroupGeometry struct {
	Count    []int64
	AABB     [][6]float32
	Centroid [][3]float64
	Cov      [][6]float64
	Eig      [][3]float64
	Axes     [][9]float64
	OBB      [][6]float64
}

// GroupStats returns the geometry of every group of a grouped id list over the tree's points (extension: no reference
// parity; include/pcgx.h, pcgx_kdtree_group_stats): ids holds group 0's members, then group 1's, and so on, sizes the
// groups' sizes -- what Clusters returns.  An id outside [0, Len()) or sizes that add up to more than len(ids) are
// ErrInvalid.
func (k *KDTree) GroupStats(ids, sizes []int64) (*GroupGeometry, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	g := len(sizes)
	r := &GroupGeometry{Count: make([]int64, g), AABB: make([][6]float32, g), Centroid: make([][3]float64, g),
		Cov: make([][6]float64, g), Eig: make([][3]float64, g), Axes: make([][9]float64, g), OBB: make([][6]float64, g)}
	if g == 0 {
		return r, nil
	}
	var pi *C.int64_t
	if len(ids) > 0 {
		pi = (*C.int64_t)(unsafe.Pointer(&ids[0]))
	}
	rc := C.pcgx_kdtree_group_stats(k.t.h, pi, C.int64_t(len(ids)), (*C.int64_t)(unsafe.Pointer(&sizes[0])), C.int64_t(g),
		(*C.int64_t)(unsafe.Pointer(&r.Count[0])), (*C.float)(unsafe.Pointer(&r.AABB[0])),
		(*C.double)(unsafe.Pointer(&r.Centroid[0])), (*C.double)(unsafe.Pointer(&r.Cov[0])),
		(*C.double)(unsafe.Pointer(&r.Eig[0])), (*C.double)(unsafe.Pointer(&r.Axes[0])),
		(*C.double)(unsafe.Pointer(&r.OBB[0])))
	runtime.KeepAlive(ids)
	runtime.KeepAlive(sizes)
	runtime.KeepAlive(r)
	if err := status(rc); err != nil {
		return nil, err
	}
	return r, nil
}

// GroupFootprints is the result of (*KDTree).GroupHulls: HullSizes per group; HullIDs, again a grouped id list (the
// vertices of group g's exact 2-D convex hull counter-clockwise from the lexicographically least place, a place by its
// smallest id, -1 behind the last hull); Area of each polygon; Rect: the minimum-area rectangle with a side along a hull
// edge as centre x, y, the unit direction u of that edge, and the half-extents along u and (-u_y, u_x).
type GroupFootprints struct {
	HullSizes []int64
	HullIDs   []int64
	Area      []float64
	Rect      [][6]float64
}

// GroupHulls returns what every group of a grouped id list stands on (extension: no reference parity; include/pcgx.h,
// pcgx_kdtree_group_hulls); ids and sizes as GroupStats takes them, and the same inputs are ErrInvalid.
func (k *KDTree) GroupHulls(ids, sizes []int64) (*GroupFootprints, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	g := len(sizes)
	r := &GroupFootprints{HullSizes: make([]int64, g), HullIDs: make([]int64, len(ids)), Area: make([]float64, g),
		Rect: make([][6]float64, g)}
	for i := range r.HullIDs {
		r.HullIDs[i] = -1
	}
	if g == 0 {
		return r, nil
	}
	var pi, ph *C.int64_t
	if len(ids) > 0 {
		pi = (*C.int64_t)(unsafe.Pointer(&ids[0]))
		ph = (*C.int64_t)(unsafe.Pointer(&r.HullIDs[0]))
	}
	rc := C.pcgx_kdtree_group_hulls(k.t.h, pi, C.int64_t(len(ids)), (*C.int64_t)(unsafe.Pointer(&sizes[0])), C.int64_t(g),
		(*C.int64_t)(unsafe.Pointer(&r.HullSizes[0])), ph, (*C.double)(unsafe.Pointer(&r.Area[0])),
		(*C.double)(unsafe.Pointer(&r.Rect[0])))
	runtime.KeepAlive(ids)
	runtime.KeepAlive(sizes)
	runtime.KeepAlive(r)
	if err := status(rc); err != nil {
		return nil, err
	}
	return r, nil
}

// FPFHMatch finds, for every row of a, the nearest usable row of b and the runner-up's distance (extension: no
// reference parity; include/pcgx.h, "FPFH matching"): float32 squared distances over the 33 values, summed left to
// right, ties to the smaller id.  ids[i] is -1 and both distances are +Inf where a's row is unusable (not finite, or
// all zero) or b has no candidate; secondDistSq[i] is +Inf with a single candidate.  Rows as FPFH returns them.
func FPFHMatch(a, b [][33]float32) (ids []int64, distSq, secondDistSq []float32, err error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	na, nb := len(a), len(b)
	ids = make([]int64, na)
	distSq = make([]float32, na)
	secondDistSq = make([]float32, na)
	if na == 0 {
		return ids, distSq, secondDistSq, nil
	}
	var pb *C.float
	if nb > 0 {
		pb = (*C.float)(unsafe.Pointer(&b[0]))
	}
	rc := C.pcgx_fpfh_match((*C.float)(unsafe.Pointer(&a[0])), C.int64_t(na), pb, C.int64_t(nb),
		(*C.int64_t)(unsafe.Pointer(&ids[0])), (*C.float)(unsafe.Pointer(&distSq[0])),
		(*C.float)(unsafe.Pointer(&secondDistSq[0])))
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	if err := status(rc); err != nil {
		return nil, nil, nil, err
	}
	return ids, distSq, secondDistSq, nil
}

// FPFHCorrespondences returns the matches of a in b as {row of a, row of b}, ascending in the row of a, that pass
// Lowe's ratio test distSq <= maxRatio^2 * secondDistSq (maxRatio in (0, 1]; 1 keeps every match) and, with mutual,
// whose row of b matches back to the same row of a (include/pcgx.h, "FPFH matching"): what feature-based coarse
// alignment estimates its pose from.
func FPFHCorrespondences(a, b [][33]float32, maxRatio float32, mutual bool) ([][2]int64, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	na, nb := len(a), len(b)
	if na == 0 {
		return nil, nil
	}
	var pb *C.float
	if nb > 0 {
		pb = (*C.float)(unsafe.Pointer(&b[0]))
	}
	src := make([]int64, na)
	dst := make([]int64, na)
	var m C.int64_t
	mu := C.int32_t(0)
	if mutual {
		mu = 1
	}
	rc := C.pcgx_fpfh_correspondences((*C.float)(unsafe.Pointer(&a[0])), C.int64_t(na), pb, C.int64_t(nb),
		C.float(maxRatio*maxRatio), mu, (*C.int64_t)(unsafe.Pointer(&src[0])), (*C.int64_t)(unsafe.Pointer(&dst[0])), &m)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	if err := status(rc); err != nil {
		return nil, err
	}
	out := make([][2]int64, int(m))
	for i := range out {
		out[i] = [2]int64{src[i], dst[i]}
	}
	return out, nil
}

// PoseResult is what PoseFromCorrespondences returns: the pose (column-major, it takes src onto dst) of the best
// hypothesis or, where Refined, the least-squares pose over its inliers; Inliers are the pairs within maxDist under it.
type PoseResult struct {
	Found, Refined  bool
	Best, BestCount int64
	Pose            [16]float32
	Inliers         []int64
}

// PoseFromCorrespondences estimates the rigid pose most pairs agree on by sample consensus on the GPU (extension: no
// reference parity; include/pcgx.h, "pose from correspondences"): pairs are {index into src, index into dst}, e.g. what
// FPFHCorrespondences returns; samples holds three random 32-bit words per hypothesis, drawn by the caller (word u
// names pair (u * m) >> 32).  edgeSimilarity in [0, 1] (0: no edge test); Found is false when no hypothesis agrees with
// three pairs.
func PoseFromCorrespondences(src, dst [][3]float32, pairs [][2]int64, samples [][3]uint32, maxDist, edgeSimilarity float32,
	refine bool) (PoseResult, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var r PoseResult
	r.Best = -1
	m, n := len(pairs), len(samples)
	s := make([]int64, m+1)
	d := make([]int64, m+1)
	ids := make([]int64, m+1)
	for k, p := range pairs {
		s[k], d[k] = p[0], p[1]
	}
	var ps, pd *C.float
	var pu *C.uint32_t
	if len(src) > 0 {
		ps = (*C.float)(unsafe.Pointer(&src[0]))
	}
	if len(dst) > 0 {
		pd = (*C.float)(unsafe.Pointer(&dst[0]))
	}
	if n > 0 {
		pu = (*C.uint32_t)(unsafe.Pointer(&samples[0]))
	}
	var found, refined C.int32_t
	var best, bestCount, nIn C.int64_t
	rf := C.int32_t(0)
	if refine {
		rf = 1
	}
	rc := C.pcgx_pose_from_correspondences(ps, C.int64_t(len(src)), pd, C.int64_t(len(dst)),
		(*C.int64_t)(unsafe.Pointer(&s[0])), (*C.int64_t)(unsafe.Pointer(&d[0])), C.int64_t(m), pu, C.int64_t(n),
		C.float(maxDist*maxDist), C.float(edgeSimilarity), rf, &found, &best, &bestCount,
		(*C.float)(unsafe.Pointer(&r.Pose[0])), &refined, &nIn, (*C.int64_t)(unsafe.Pointer(&ids[0])), nil, nil, nil)
	runtime.KeepAlive(src)
	runtime.KeepAlive(dst)
	runtime.KeepAlive(samples)
	if err := status(rc); err != nil {
		return PoseResult{}, err
	}
	r.Found, r.Refined = found != 0, refined != 0
	r.Best, r.BestCount = int64(best), int64(bestCount)
	r.Inliers = ids[:int(nIn)]
	return r, nil
}

// ScoreResult is what ScorePoses returns: per pose the number of source points that land within maxDist of the tree's
// cloud and the float64 sum of their DistSq; Best is the live pose with the largest count (the smallest index among
// equals, -1 if no pose is live: a pose of sixteen zeros is dead) and Pose its sixteen numbers.
type ScoreResult struct {
	Counts []int64
	Sums   []float64
	Best   int64
	Pose   [16]float32
}

// ScorePoses scores poses (column-major, each takes src onto the tree's cloud) on the whole clouds in one call
// (extension: no reference parity; include/pcgx.h, "score poses"): the verification a pose picked from correspondences
// alone needs on scenes with repeated structure.
func (k *KDTree) ScorePoses(src []mat.Vec3, poses [][16]float32, maxDist float32) (ScoreResult, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var r ScoreResult
	r.Best = -1
	n, np := len(src), len(poses)
	r.Counts = make([]int64, np)
	r.Sums = make([]float64, np)
	var ps, pm *C.float
	var pc *C.int64_t
	var pd *C.double
	if n > 0 {
		ps = (*C.float)(unsafe.Pointer(&src[0]))
	}
	if np > 0 {
		pm = (*C.float)(unsafe.Pointer(&poses[0]))
		pc = (*C.int64_t)(unsafe.Pointer(&r.Counts[0]))
		pd = (*C.double)(unsafe.Pointer(&r.Sums[0]))
	}
	var best C.int64_t
	rc := C.pcgx_kdtree_score_poses(k.t.h, ps, C.int64_t(n), pm, C.int64_t(np), C.float(maxDist), pc, pd, &best,
		(*C.float)(unsafe.Pointer(&r.Pose[0])))
	runtime.KeepAlive(src)
	runtime.KeepAlive(poses)
	if err := status(rc); err != nil {
		return ScoreResult{}, err
	}
	r.Best = int64(best)
	return r, nil
}

// PoseSelect picks the k best hypotheses of a pose estimation for ScorePoses (include/pcgx.h, pcgx_pose_select): status 0
// and count >= 3, by count descending, then by index; ids[j] and poses[j], -1 and a dead pose behind the last one.
func PoseSelect(hypStatus []int32, counts []int64, poses [][16]float32, k int) (ids []int64, out [][16]float32, selected int, err error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	n := len(hypStatus)
	if len(counts) != n || len(poses) != n {
		return nil, nil, 0, errors.New("pcgx: status, counts and poses must have one entry per hypothesis")
	}
	if k < 0 {
		k = 0
	}
	ids = make([]int64, k)
	out = make([][16]float32, k)
	var pst *C.int32_t
	var pct, pid *C.int64_t
	var pps, pout *C.float
	if n > 0 {
		pst = (*C.int32_t)(unsafe.Pointer(&hypStatus[0]))
		pct = (*C.int64_t)(unsafe.Pointer(&counts[0]))
		pps = (*C.float)(unsafe.Pointer(&poses[0]))
	}
	if k > 0 {
		pid = (*C.int64_t)(unsafe.Pointer(&ids[0]))
		pout = (*C.float)(unsafe.Pointer(&out[0]))
	}
	var nSel C.int64_t
	rc := C.pcgx_pose_select(pst, pct, pps, C.int64_t(n), C.int64_t(k), pid, pout, &nSel)
	runtime.KeepAlive(hypStatus)
	runtime.KeepAlive(counts)
	runtime.KeepAlive(poses)
	if err := status(rc); err != nil {
		return nil, nil, 0, err
	}
	return ids, out, int(nSel), nil
}

// Covariance modes of KDTree.Covariances (include/pcgx.h, pcgx_kdtree_covariances).
const (
	CovRaw   = int(C.PCGX_COV_RAW)   // the covariance as it is
	CovPlane = int(C.PCGX_COV_PLANE) // I - (1 - epsilon) u u^T: Generalized ICP's regularised plane
)

// Covariances returns the covariance of every query's kk nearest neighbours (KNearestBatch's lists; extension: no
// reference parity; include/pcgx.h, pcgx_kdtree_covariances) as xx, xy, xz, yy, yz, zz, the unit normal u of the
// neighbourhood turned towards viewpoint, and the neighbour count.  mode CovPlane gives I - (1 - epsilon) u u^T,
// CovRaw the covariance as it is; fewer than 3 neighbours, or all at one place, give I / 0 and a zero normal.
// q == nil takes the tree's own points, in id order.
func (k *KDTree) Covariances(q []mat.Vec3, kk int, maxRange float32, mode int, epsilon float32, viewpoint mat.Vec3) ([][6]float32, []mat.Vec3, []int32, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var qp *C.float
	n := len(q)
	if q == nil {
		var ln C.int64_t
		if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
			return nil, nil, nil, err
		}
		n = int(ln)
	} else if n > 0 {
		qp = (*C.float)(unsafe.Pointer(&q[0]))
	}
	cov := make([][6]float32, n)
	normals := make([]mat.Vec3, n)
	counts := make([]int32, n)
	if n == 0 {
		return cov, normals, counts, nil
	}
	vp := viewpoint
	rc := C.pcgx_kdtree_covariances(k.t.h, qp, C.int64_t(n), C.int32_t(kk), C.float(maxRange), C.int32_t(mode),
		C.float(epsilon), (*C.float)(unsafe.Pointer(&vp[0])), (*C.float)(unsafe.Pointer(&cov[0][0])),
		(*C.float)(unsafe.Pointer(&normals[0])), (*C.int32_t)(unsafe.Pointer(&counts[0])))
	runtime.KeepAlive(q)
	runtime.KeepAlive(cov)
	runtime.KeepAlive(normals)
	runtime.KeepAlive(counts)
	if err := status(rc); err != nil {
		return nil, nil, nil, err
	}
	return cov, normals, counts, nil
}

// KNearest returns the kk points of the tree with the smallest (DistSq, ID) among those with DistSq < maxRange^2,
// ascending (extension: no reference parity; include/pcgx.h, pcgx_kdtree_knearest: ties go by ID).  Like Nearest it
// is one blocking GPU call and panics where the call fails (kk outside [1, 64], a NaN maxRange).
func (k *KDTree) KNearest(p mat.Vec3, kk int, maxRange float32) []storage.Neighbor {
	atomic.AddInt64(&singlePointCalls, 1)
	r, err := k.KNearestBatch([]mat.Vec3{p}, kk, maxRange)
	if err != nil {
		panic(err)
	}
	return r[0]
}

// KNearestBatch is KNearest for every query, one row each (at most kk long); q == nil takes the tree's own points,
// in id order.
func (k *KDTree) KNearestBatch(q []mat.Vec3, kk int, maxRange float32) ([][]storage.Neighbor, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	var qp *C.float
	n := len(q)
	if q == nil {
		var ln C.int64_t
		if err := status(C.pcgx_kdtree_len(k.t.h, &ln)); err != nil {
			return nil, err
		}
		n = int(ln)
	} else if n > 0 {
		qp = (*C.float)(unsafe.Pointer(&q[0]))
	}
	if n == 0 {
		return [][]storage.Neighbor{}, nil
	}
	if kk < 1 || kk > 64 {
		return nil, errors.New("pcgx: k must be in [1, 64]")
	}
	ids := make([]int64, n*kk)
	dsq := make([]float32, n*kk)
	counts := make([]int32, n)
	rc := C.pcgx_kdtree_knearest(k.t.h, qp, C.int64_t(n), C.int32_t(kk), C.float(maxRange),
		(*C.int64_t)(unsafe.Pointer(&ids[0])), (*C.float)(unsafe.Pointer(&dsq[0])), (*C.int32_t)(unsafe.Pointer(&counts[0])))
	runtime.KeepAlive(q)
	if err := status(rc); err != nil {
		return nil, err
	}
	out := make([][]storage.Neighbor, n)
	for i := range out {
		row := make([]storage.Neighbor, counts[i])
		for s := range row {
			row[s] = storage.Neighbor{ID: int(ids[i*kk+s]), DistSq: dsq[i*kk+s]}
		}
		out[i] = row
	}
	return out, nil
}

// Nearest keeps storage.Search working for single points (one tiny batch).
func (k *KDTree) Nearest(p mat.Vec3, maxRange float32) storage.Neighbor {
	atomic.AddInt64(&singlePointCalls, 1)
	r, err := k.NearestBatch([]mat.Vec3{p}, maxRange)
	if err != nil {
		panic(err)
	}
	return r[0]
}

// RangeBatch: neighbours with DistSq < maxRange^2 of every query, each list sorted by DistSq
// (KDTree.Range, kdtree.go:148-161).  out[i] belongs to q[i].
func (k *KDTree) RangeBatch(q []mat.Vec3, maxRange float32) ([][]storage.Neighbor, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k) // the finalizer must not free the handle while a call is in flight
	n := len(q)
	out := make([][]storage.Neighbor, n)
	if n == 0 {
		return out, nil
	}
	counts := make([]int64, n)
	qp := (*C.float)(unsafe.Pointer(&q[0]))
	if err := status(C.pcgx_kdtree_range_count(k.t.h, qp, C.int64_t(n), C.float(maxRange),
		(*C.int64_t)(unsafe.Pointer(&counts[0])))); err != nil {
		return nil, err
	}
	offs := make([]int64, n+1)
	for i, c := range counts {
		offs[i+1] = offs[i] + c
	}
	total := offs[n]
	ids := make([]int64, total+1)
	dsq := make([]float32, total+1)
	if err := status(C.pcgx_kdtree_range_fill(k.t.h, qp, C.int64_t(n), C.float(maxRange),
		(*C.int64_t)(unsafe.Pointer(&offs[0])), (*C.int64_t)(unsafe.Pointer(&ids[0])),
		(*C.float)(unsafe.Pointer(&dsq[0])))); err != nil {
		return nil, err
	}
	for i := range out {
		nb := make([]storage.Neighbor, counts[i])
		for j := range nb {
			nb[j] = storage.Neighbor{ID: int(ids[offs[i]+int64(j)]), DistSq: dsq[offs[i]+int64(j)]}
		}
		out[i] = nb
	}
	return out, nil
}

// Range keeps storage.Search working for single points.
func (k *KDTree) Range(p mat.Vec3, maxRange float32) []storage.Neighbor {
	atomic.AddInt64(&singlePointCalls, 1)
	r, err := k.RangeBatch([]mat.Vec3{p}, maxRange)
	if err != nil {
		panic(err)
	}
	return r[0]
}

// -------------------------------------------------------------- VoxelGrid

type voxelGrid struct {
	leaf  mat.Vec3
	chunk [3]int
}

// NewVoxelGrid replaces voxelgrid.New(leaf, WithChunkSize(chunk))
// (pc/filter/voxelgrid/voxelgrid.go:23-33); chunk {0,0,0} = non-chunked.
func NewVoxelGrid(leaf mat.Vec3, chunk [3]int) filter.Filter {
	return &voxelGrid{leaf: leaf, chunk: chunk}
}

func (f *voxelGrid) Filter(pp *pc.PointCloud) (*pc.PointCloud, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(f) // the finalizer must not free the handle while a call is in flight
	stride, off, err := xyzLayout(pp)
	if err != nil {
		return nil, err
	}
	n := pp.Points
	if n == 0 {
		return nil, errors.New("no point")
	}
	out := make([]byte, n*stride)
	leaf := [3]C.float{C.float(f.leaf[0]), C.float(f.leaf[1]), C.float(f.leaf[2])}
	chunk := [3]C.int32_t{C.int32_t(f.chunk[0]), C.int32_t(f.chunk[1]), C.int32_t(f.chunk[2])}
	var m C.int64_t
	rc := C.pcgx_voxel_filter(unsafe.Pointer(&pp.Data[0]), C.int64_t(n), C.int32_t(stride), C.int32_t(off),
		&leaf[0], &chunk[0], unsafe.Pointer(&out[0]), &m)
	if err := status(rc); err != nil {
		return nil, err
	}
	newPc := &pc.PointCloud{PointCloudHeader: pp.Clone(), Points: int(m), Data: out[:int(m)*stride]}
	newPc.Width, newPc.Height = int(m), 1
	return newPc, nil
}

// ---------------------------------------------- statistical outlier removal (extension)

// SOR is a filter.Filter for statistical outlier removal (no reference counterpart; PCL's
// StatisticalOutlierRemoval; include/pcgx.h, pcgx_sor_filter): keeps the points whose mean distance to their MeanK
// nearest other finite points is at most mu + StddevMul * sigma (Negative: the others), records byte for byte in
// input order.  Non-finite points are dropped in both modes.
type SOR struct {
	MeanK     int
	StddevMul float32
	Negative  bool
}

// Filter runs the filter; Stats is the same with the mean distances (by input index, NaN for dropped points) and
// {mu, sigma, threshold}.
func (f *SOR) Filter(pp *pc.PointCloud) (*pc.PointCloud, error) {
	out, _, _, err := f.FilterStats(pp)
	return out, err
}

func (f *SOR) FilterStats(pp *pc.PointCloud) (*pc.PointCloud, []float64, [3]float64, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	var stats [3]float64
	stride, off, err := xyzLayout(pp)
	if err != nil {
		return nil, nil, stats, err
	}
	n := pp.Points
	if n == 0 {
		return nil, nil, stats, errors.New("no point")
	}
	out := make([]byte, n*stride)
	md := make([]float64, n)
	neg := C.int32_t(0)
	if f.Negative {
		neg = 1
	}
	var m C.int64_t
	rc := C.pcgx_sor_filter(unsafe.Pointer(&pp.Data[0]), C.int64_t(n), C.int32_t(stride), C.int32_t(off),
		C.int32_t(f.MeanK), C.float(f.StddevMul), neg, unsafe.Pointer(&out[0]), &m,
		(*C.double)(unsafe.Pointer(&md[0])), (*C.double)(unsafe.Pointer(&stats[0])))
	runtime.KeepAlive(pp)
	if err := status(rc); err != nil {
		return nil, nil, stats, err
	}
	newPc := &pc.PointCloud{PointCloudHeader: pp.Clone(), Points: int(m), Data: out[:int(m)*stride]}
	newPc.Width, newPc.Height = int(m), 1
	return newPc, md, stats, nil
}

// ROR is a filter.Filter for radius outlier removal (no reference counterpart; PCL's RadiusOutlierRemoval;
// include/pcgx.h, pcgx_ror_filter): keeps the finite points with at least MinNeighbors finite points within Radius,
// themselves included (Negative: the other finite points), records byte for byte in input order.  Non-finite points
// are dropped in both modes.
type ROR struct {
	Radius       float32
	MinNeighbors int
	Negative     bool
}

func (f *ROR) Filter(pp *pc.PointCloud) (*pc.PointCloud, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	stride, off, err := xyzLayout(pp)
	if err != nil {
		return nil, err
	}
	n := pp.Points
	if n == 0 {
		return nil, errors.New("no point")
	}
	out := make([]byte, n*stride)
	neg := C.int32_t(0)
	if f.Negative {
		neg = 1
	}
	var m C.int64_t
	rc := C.pcgx_ror_filter(unsafe.Pointer(&pp.Data[0]), C.int64_t(n), C.int32_t(stride), C.int32_t(off),
		C.float(f.Radius), C.int32_t(f.MinNeighbors), neg, unsafe.Pointer(&out[0]), &m)
	runtime.KeepAlive(pp)
	if err := status(rc); err != nil {
		return nil, err
	}
	newPc := &pc.PointCloud{PointCloudHeader: pp.Clone(), Points: int(m), Data: out[:int(m)*stride]}
	newPc.Width, newPc.Height = int(m), 1
	return newPc, nil
}

// FilterSharded is this rank's share of Filter(pp) over the ranks of c (SURVEY 8(e)): every rank
// passes the same cloud; the ranks' results, rank 0's first, are Filter's output record for record.
// Collective.
func FilterSharded(f filter.Filter, pp *pc.PointCloud, c *Comm) (*pc.PointCloud, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(c)
	vg, ok := f.(*voxelGrid)
	if !ok {
		return nil, errors.New("pcgx: FilterSharded needs a filter made by NewVoxelGrid")
	}
	stride, off, err := xyzLayout(pp)
	if err != nil {
		return nil, err
	}
	n := pp.Points
	if n == 0 {
		return nil, errors.New("no point")
	}
	out := make([]byte, n*stride)
	leaf := [3]C.float{C.float(vg.leaf[0]), C.float(vg.leaf[1]), C.float(vg.leaf[2])}
	chunk := [3]C.int32_t{C.int32_t(vg.chunk[0]), C.int32_t(vg.chunk[1]), C.int32_t(vg.chunk[2])}
	var m C.int64_t
	rc := C.pcgx_voxel_filter_sharded(c.h, unsafe.Pointer(&pp.Data[0]), C.int64_t(n), C.int32_t(stride), C.int32_t(off),
		&leaf[0], &chunk[0], unsafe.Pointer(&out[0]), &m)
	if err := status(rc); err != nil {
		return nil, err
	}
	part := &pc.PointCloud{PointCloudHeader: pp.Clone(), Points: int(m), Data: out[:int(m)*stride]}
	part.Width, part.Height = int(m), 1
	return part, nil
}

// -------------------------------------------------------------------- ICP

// Evaluator implements icp.Evaluator with the fused GPU correspondence +
// reduction (replaces PointToPointEvaluator + NearestPointCorresponder,
// evaluator.go:91-189, correspondence.go:22-37; default weight only).
type Evaluator struct {
	MaxDist  float32
	MinPairs int
	// Weight replaces PointToPointEvaluator.WeightFn (evaluator.go:72): the reference accepts any Go
	// closure, the device one of the built-in forms below.  Weight.Func() is the matching closure
	// for the CPU evaluator, so both compute the same float32 weights.  Zero value: w = 1.
	Weight WeightFn
	// Sums selects how the nine sums of evaluator.go:122-145 are formed (include/pcgx.h PCGX_SUMS_*).
	// Zero value SumsReference: the reference's own sequential float32 additions, evaluated exactly by
	// the whole GPU -- Evaluate and Fit return what the CPU code returns, bit for bit, at any size.
	// SumsF64Tree: a fixed-order float64 reduction of the same terms (about 3x faster per iteration at
	// 1M pairs; differs from the reference by the reference's own rounding noise, 1.6e-5 on the pose
	// at 1M pairs); it is what FitSharded computes when the target is spread over several ranks.
	Sums int
}

// Evaluator.Sums (include/pcgx.h PCGX_SUMS_*).
const (
	SumsReference      = 0
	SumsF64Tree        = 1
	SumsReferenceChain = 2 // one wave adding term after term: the on-device cross-check
)

// WeightFn kinds (include/pcgx.h PCGX_WEIGHT_*).
const (
	WeightOne      = 0 // DefaultEvaluateWeightFn
	WeightConstant = 1 // a
	WeightInverse  = 2 // 1 / (a + d)
	WeightHuber    = 3 // d <= a ? 1 : sqrt(a / d)
	WeightTukey    = 4 // d < a ? (1 - d/a)^2 : 0
)

type WeightFn struct {
	Kind int
	A    float32
}

// Func is the closure icp.PointToPointEvaluator{WeightFn: ...} takes for the same weights on the CPU.
func (w WeightFn) Func() icp.EvaluateWeightFn {
	a := w.A
	switch w.Kind {
	case WeightConstant:
		return func(float32) float32 { return a }
	case WeightInverse:
		return func(d float32) float32 { return 1 / (a + d) }
	case WeightHuber:
		return func(d float32) float32 {
			if d <= a {
				return 1
			}
			return float32(math.Sqrt(float64(a / d)))
		}
	case WeightTukey:
		return func(d float32) float32 {
			if !(d < a) {
				return 0
			}
			u := 1 - d/a
			return u * u
		}
	}
	return icp.DefaultEvaluateWeightFn
}

var _ icp.Evaluator = (*Evaluator)(nil)

func (Evaluator) HasGradient() bool { return true }
func (Evaluator) HasHessian() bool  { return false }

func packVec3(ra pc.Vec3RandomAccessor) []float32 {
	if s, ok := ra.(pc.Vec3Slice); ok && len(s) > 0 {
		return unsafe.Slice((*float32)(unsafe.Pointer(&s[0])), 3*len(s))
	}
	out := make([]float32, 3*ra.Len())
	for i := 0; i < ra.Len(); i++ {
		v := ra.Vec3At(i)
		copy(out[3*i:], v[:])
	}
	return out
}

func (e *Evaluator) Evaluate(base storage.Search, target pc.Vec3RandomAccessor) (*icp.Evaluated, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(e) // the finalizer must not free the handle while a call is in flight
	k, ok := base.(*KDTree)
	if !ok {
		return nil, errors.New("pcgx: base must be a *pcgx.KDTree")
	}
	t := packVec3(target)
	var tp *C.float
	if len(t) > 0 {
		tp = (*C.float)(unsafe.Pointer(&t[0]))
	}
	var ev C.pcgx_icp_evaluated
	var p C.pcgx_icp_params
	p.max_dist, p.min_dist_sq, p.min_pairs = C.float(e.MaxDist), C.float(k.MinDistSq), C.int32_t(e.MinPairs)
	p.weight_fn, p.weight_fn_param = C.int32_t(e.Weight.Kind), C.float(e.Weight.A)
	p.sums_mode = C.int32_t(e.Sums)
	rc := C.pcgx_icp_evaluate_params(k.t.h, tp, C.int64_t(target.Len()), &p, &ev)
	runtime.KeepAlive(k)
	if err := status(rc); err != nil {
		return nil, err
	}
	out := &icp.Evaluated{Value: float32(ev.value), DistRMS: float32(ev.dist_rms)}
	for i := 0; i < 6; i++ {
		out.Gradient[i] = float32(ev.gradient[i])
	}
	return out, nil
}

// Corresponder implements icp.PointToPointCorresponder (correspondence.go:14-16) over pcgx_icp_pairs: one batched
// nearest-neighbour pass for all targets, the pairs compacted in target order exactly as
// NearestPointCorresponder.Pairs emits them (correspondence.go:22-37).  The reference's own
// icp.PointToPointEvaluator{Corresponder: &pcgx.Corresponder{MaxDist: d}} then runs its CPU reduction (and any Go
// WeightFn closure) over GPU correspondences.  A base that is not a *pcgx.KDTree is answered by the reference's
// loop over base.Nearest.
type Corresponder struct {
	MaxDist float32
}

var _ icp.PointToPointCorresponder = (*Corresponder)(nil)

func (c *Corresponder) Pairs(base storage.Search, target pc.Vec3RandomAccessor) []icp.PointToPointCorrespondence {
	k, ok := base.(*KDTree)
	if !ok {
		return (&icp.NearestPointCorresponder{MaxDist: c.MaxDist}).Pairs(base, target)
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(k)
	n := target.Len()
	if n == 0 {
		return []icp.PointToPointCorrespondence{}
	}
	t := packVec3(target)
	baseID := make([]int64, n)
	targetID := make([]int64, n)
	dsq := make([]float32, n)
	var np C.int64_t
	rc := C.pcgx_icp_pairs(k.t.h, (*C.float)(unsafe.Pointer(&t[0])), C.int64_t(n), C.float(c.MaxDist), C.float(k.MinDistSq),
		(*C.int64_t)(unsafe.Pointer(&baseID[0])), (*C.int64_t)(unsafe.Pointer(&targetID[0])), (*C.float)(unsafe.Pointer(&dsq[0])), &np)
	if err := status(rc); err != nil {
		panic(err) // the interface has no error result; the reference's loop cannot fail either
	}
	out := make([]icp.PointToPointCorrespondence, int(np))
	for i := range out {
		out[i] = icp.PointToPointCorrespondence{BaseID: int(baseID[i]), TargetID: int(targetID[i]), SquaredDistance: dsq[i]}
	}
	return out
}

// Fit runs the whole PointToPointICPGradient.Fit loop on the device
// (icp.go:23-67) with a GradientDescentUpdaterFactory's parameters.
func Fit(base *KDTree, target pc.Vec3RandomAccessor, e *Evaluator, u *icp.GradientDescentUpdaterFactory) (mat.Mat4, icp.Stat, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(base)
	var p C.pcgx_icp_params
	p.max_dist, p.min_dist_sq, p.min_pairs = C.float(e.MaxDist), C.float(base.MinDistSq), C.int32_t(e.MinPairs)
	p.weight_fn, p.weight_fn_param = C.int32_t(e.Weight.Kind), C.float(e.Weight.A)
	p.sums_mode = C.int32_t(e.Sums)
	if u != nil {
		for i := 0; i < 6; i++ {
			p.weight[i], p.threshold[i] = C.float(u.Weight[i]), C.float(u.Threshold[i])
		}
		p.max_iteration = C.int32_t(u.MaxIteration)
	}
	t := packVec3(target)
	var tp *C.float
	if len(t) > 0 {
		tp = (*C.float)(unsafe.Pointer(&t[0]))
	}
	var trans mat.Mat4
	var st C.pcgx_icp_stat
	rc := C.pcgx_icp_fit(base.t.h, tp, C.int64_t(target.Len()), &p, (*C.float)(unsafe.Pointer(&trans[0])), &st)
	stat := icp.Stat{NumIteration: int(st.num_iteration)}
	stat.Value, stat.DistRMS = float32(st.evaluated.value), float32(st.evaluated.dist_rms)
	for i := 0; i < 6; i++ {
		stat.Gradient[i] = float32(st.evaluated.gradient[i])
	}
	return trans, stat, status(rc)
}

// ------------------------------------------ point-to-plane ICP (extension)

// ErrSingular: the 6x6 normal equations are not positive definite.
var ErrSingular = errors.New("pcgx: normal equations are not positive definite")

// PlaneEvaluator fills the slots the reference leaves empty (Evaluated.Hessian,
// HasHessian(), evaluator.go:28,35,76): point-to-plane residual r = n.(pt-pb),
// J = {n, pt x n}, Hessian = 2/sum(w) * sum J J^T.  BaseNormals holds one unit
// normal per base point in the tree's id order.  No counterpart in the reference.
type PlaneEvaluator struct {
	MaxDist     float32
	MinPairs    int
	BaseNormals []mat.Vec3
}

var _ icp.Evaluator = (*PlaneEvaluator)(nil)

func (PlaneEvaluator) HasGradient() bool { return true }
func (PlaneEvaluator) HasHessian() bool  { return true }

// Evaluate runs one fused correspondence + 30-sum reduction on the device.
func (e *PlaneEvaluator) Evaluate(base storage.Search, target pc.Vec3RandomAccessor) (*icp.Evaluated, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(e) // the finalizer must not free the handle while a call is in flight
	k, ok := base.(*KDTree)
	if !ok {
		return nil, errors.New("pcgx: base must be a *pcgx.KDTree")
	}
	if len(e.BaseNormals) != k.Len() || len(e.BaseNormals) == 0 {
		return nil, errors.New("pcgx: one normal per base point is required")
	}
	t := packVec3(target)
	var tp *C.float
	if len(t) > 0 {
		tp = (*C.float)(unsafe.Pointer(&t[0]))
	}
	var p C.pcgx_icp_params
	p.max_dist, p.min_pairs = C.float(e.MaxDist), C.int32_t(e.MinPairs)
	var s *C.pcgx_icp_session
	rc := C.pcgx_icp_plane_session_create(k.t.h, (*C.float)(unsafe.Pointer(&e.BaseNormals[0])), tp,
		C.int64_t(target.Len()), 0, &p, 0, nil, &s)
	if err := status(rc); err != nil {
		return nil, err
	}
	defer C.pcgx_icp_session_free(s)
	if err := status(C.pcgx_icp_session_partials(s, nil)); err != nil {
		return nil, err
	}
	var sums [30]C.double
	if err := status(C.pcgx_icp_session_read_sums_n(s, &sums[0], 30, nil)); err != nil {
		return nil, err
	}
	var ev C.pcgx_icp_evaluated
	out := &icp.Evaluated{}
	rc = C.pcgx_icp_plane_finish_evaluate(&sums[0], C.int32_t(e.MinPairs), &ev, (*C.float)(unsafe.Pointer(&out.Hessian[0])))
	if err := status(rc); err != nil {
		return nil, err
	}
	out.Value = float32(ev.value)
	for i := 0; i < 6; i++ {
		out.Gradient[i] = float32(ev.gradient[i])
	}
	return out, nil
}

// FitPlane runs the whole loop (icp.go:23-67 shape) with the point-to-plane
// evaluator and a Gauss-Newton updater on the device.
func FitPlane(base *KDTree, target pc.Vec3RandomAccessor, e *PlaneEvaluator, threshold mat.Vec6, maxIteration int, damping float32) (mat.Mat4, icp.Stat, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(base)
	var p C.pcgx_icp_params
	p.max_dist, p.min_pairs, p.max_iteration = C.float(e.MaxDist), C.int32_t(e.MinPairs), C.int32_t(maxIteration)
	for i := 0; i < 6; i++ {
		p.threshold[i] = C.float(threshold[i])
	}
	t := packVec3(target)
	var tp *C.float
	if len(t) > 0 {
		tp = (*C.float)(unsafe.Pointer(&t[0]))
	}
	var trans mat.Mat4
	var st C.pcgx_icp_stat
	stat := icp.Stat{}
	if len(e.BaseNormals) != base.Len() || len(e.BaseNormals) == 0 {
		return trans, stat, errors.New("pcgx: one normal per base point is required")
	}
	rc := C.pcgx_icp_plane_fit(base.t.h, (*C.float)(unsafe.Pointer(&e.BaseNormals[0])), tp, C.int64_t(target.Len()), &p,
		C.float(damping), (*C.float)(unsafe.Pointer(&trans[0])), &st, (*C.float)(unsafe.Pointer(&stat.Hessian[0])))
	stat.NumIteration = int(st.num_iteration)
	stat.Value = float32(st.evaluated.value)
	for i := 0; i < 6; i++ {
		stat.Gradient[i] = float32(st.evaluated.gradient[i])
	}
	if rc == C.PCGX_E_SINGULAR {
		return trans, stat, ErrSingular
	}
	return trans, stat, status(rc)
}

// ------------------------------------------ Generalized ICP (extension)

// GICP is Generalized ICP (Segal, Haehnel, Thrun 2009; include/pcgx.h "Generalized ICP"): the residual r = p - b of
// each nearest-point pair weighed by (C_b + R C_t R^T)^-1, Gauss-Newton on the same 6x6 normal equations as the
// point-to-plane extension.  No counterpart in the reference.  Pairs whose covariances cannot be inverted are dropped
// and do not count as pairs.
type GICP struct {
	MaxDist      float32
	MinPairs     int
	Threshold    mat.Vec6
	MaxIteration int
	Damping      float32
}

func (g *GICP) params() C.pcgx_icp_params {
	var p C.pcgx_icp_params
	p.max_dist, p.min_pairs, p.max_iteration = C.float(g.MaxDist), C.int32_t(g.MinPairs), C.int32_t(g.MaxIteration)
	for i := 0; i < 6; i++ {
		p.threshold[i] = C.float(g.Threshold[i])
	}
	return p
}

func gicpStat(st *C.pcgx_icp_stat, stat *icp.Stat, rc C.pcgx_status) error {
	stat.NumIteration = int(st.num_iteration)
	stat.Value = float32(st.evaluated.value)
	for i := 0; i < 6; i++ {
		stat.Gradient[i] = float32(st.evaluated.gradient[i])
	}
	if rc == C.PCGX_E_SINGULAR {
		return ErrSingular
	}
	return status(rc)
}

// Fit takes the covariances from the caller: baseCov per base point in the tree's id order, targetCov per target
// point in the target's own frame, each xx, xy, xz, yy, yz, zz (KDTree.Covariances of a tree over each cloud).
func (g *GICP) Fit(base *KDTree, baseCov [][6]float32, target pc.Vec3RandomAccessor, targetCov [][6]float32) (mat.Mat4, icp.Stat, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(base)
	var trans mat.Mat4
	stat := icp.Stat{}
	if len(baseCov) != base.Len() || len(baseCov) == 0 || len(targetCov) != target.Len() || len(targetCov) == 0 {
		return trans, stat, errors.New("pcgx: one covariance per base point and per target point is required")
	}
	p := g.params()
	t := packVec3(target)
	var st C.pcgx_icp_stat
	rc := C.pcgx_icp_gicp_fit(base.t.h, (*C.float)(unsafe.Pointer(&baseCov[0][0])), (*C.float)(unsafe.Pointer(&t[0])),
		(*C.float)(unsafe.Pointer(&targetCov[0][0])), C.int64_t(target.Len()), &p, C.float(g.Damping),
		(*C.float)(unsafe.Pointer(&trans[0])), &st, (*C.float)(unsafe.Pointer(&stat.Hessian[0])))
	runtime.KeepAlive(baseCov)
	runtime.KeepAlive(targetCov)
	return trans, stat, gicpStat(&st, &stat, rc)
}

// FitKNN is the one call: both clouds' regularised-plane covariances from their k nearest neighbours (CovPlane,
// epsilon, neighbours within covMaxRange) are computed on the device and never leave it.
func (g *GICP) FitKNN(base *KDTree, target pc.Vec3RandomAccessor, k int, covMaxRange, epsilon float32) (mat.Mat4, icp.Stat, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(base)
	var trans mat.Mat4
	stat := icp.Stat{}
	p := g.params()
	t := packVec3(target)
	var tp *C.float
	if len(t) > 0 {
		tp = (*C.float)(unsafe.Pointer(&t[0]))
	}
	var st C.pcgx_icp_stat
	rc := C.pcgx_icp_gicp_fit_knn(base.t.h, tp, C.int64_t(target.Len()), C.int32_t(k), C.float(covMaxRange), C.float(epsilon),
		&p, C.float(g.Damping), (*C.float)(unsafe.Pointer(&trans[0])), &st, (*C.float)(unsafe.Pointer(&stat.Hessian[0])))
	return trans, stat, gicpStat(&st, &stat, rc)
}

// ------------------------------------------------- bucket grid, segmentation

// BucketGrid is pc/storage/voxelgrid.VoxelGrid filled with Add(point i, i) for
// a whole cloud (voxelgrid.go:15-23,37-45), with pc/segmentation/voxelgrid's
// Segment (voxelgrid.go:39-73) answered from the connected components the
// device computes for the whole grid.
type BucketGrid struct {
	h *C.pcgx_bucket_grid
}

// NewBucketGrid builds the grid over every point of ra.
func NewBucketGrid(resolution float32, size [3]int, origin mat.Vec3, ra pc.Vec3RandomAccessor) (*BucketGrid, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	xyz := packVec3(ra)
	var data unsafe.Pointer
	if len(xyz) > 0 {
		data = unsafe.Pointer(&xyz[0])
	}
	sz := [3]C.int64_t{C.int64_t(size[0]), C.int64_t(size[1]), C.int64_t(size[2])}
	g := &BucketGrid{}
	rc := C.pcgx_bucket_grid_build(data, C.int64_t(ra.Len()), 12, 0, C.float(resolution), &sz[0],
		(*C.float)(unsafe.Pointer(&origin[0])), &g.h)
	if err := status(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(g, func(g *BucketGrid) { g.Close() })
	return g, nil
}

// Close releases the grid.
func (g *BucketGrid) Close() {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(g) // the finalizer must not free the handle while a call is in flight
	if g.h != nil {
		C.pcgx_bucket_grid_free(g.h)
		g.h = nil
	}
}

func idsToInt(ids []int64) []int {
	out := make([]int, len(ids))
	for i, v := range ids {
		out[i] = int(v)
	}
	return out
}

// Get returns the ids of p's voxel, nil when p is outside the grid (voxelgrid.go:52-58).
func (g *BucketGrid) Get(p mat.Vec3) []int {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(g) // the finalizer must not free the handle while a call is in flight
	var cnt C.int64_t
	if C.pcgx_bucket_grid_get(g.h, (*C.float)(unsafe.Pointer(&p[0])), nil, 0, &cnt) != C.PCGX_OK || cnt < 0 {
		return nil
	}
	ids := make([]int64, int(cnt)+1)
	C.pcgx_bucket_grid_get(g.h, (*C.float)(unsafe.Pointer(&p[0])), (*C.int64_t)(unsafe.Pointer(&ids[0])), cnt, &cnt)
	return idsToInt(ids[:int(cnt)])
}

// Segment is segmentation/voxelgrid.VoxelGrid.Segment, ids in the reference's own order.
func (g *BucketGrid) Segment(p mat.Vec3) []int {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(g) // the finalizer must not free the handle while a call is in flight
	var cnt C.int64_t
	if C.pcgx_bucket_grid_segment_bfs(g.h, (*C.float)(unsafe.Pointer(&p[0])), nil, 0, &cnt) != C.PCGX_OK || cnt <= 0 {
		return nil
	}
	ids := make([]int64, int(cnt))
	C.pcgx_bucket_grid_segment_bfs(g.h, (*C.float)(unsafe.Pointer(&p[0])), (*C.int64_t)(unsafe.Pointer(&ids[0])), cnt, &cnt)
	return idsToInt(ids[:int(cnt)])
}

// RegionGrowing is pc/segmentation/regiongrowing.RegionGrowing (regiongrowing.go:13-56) with the
// regions of the whole cloud labelled on the device once per maxRange.
type RegionGrowing struct {
	search   *KDTree
	labels   []uint32
	comp     []int64
	maxRange float32
}

// NewRegionGrowing mirrors regiongrowing.New(search, propertyIter).
func NewRegionGrowing(search *KDTree, propertyIter pc.Uint32RandomAccessor) *RegionGrowing {
	labels := make([]uint32, search.Len())
	for i := range labels {
		labels[i] = propertyIter.Uint32At(i)
	}
	return &RegionGrowing{search: search, labels: labels}
}

// Segment mirrors RegionGrowing.Segment, ids in the reference's own order.
func (r *RegionGrowing) Segment(p mat.Vec3, maxRange float32) []int {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(r) // the finalizer must not free the handle while a call is in flight
	n := len(r.labels)
	if n == 0 {
		return []int{}
	}
	ids := make([]int64, n)
	var cnt C.int64_t
	if C.pcgx_region_growing_segment_bfs(r.search.t.h, (*C.uint32_t)(unsafe.Pointer(&r.labels[0])),
		(*C.float)(unsafe.Pointer(&p[0])), C.float(maxRange), (*C.int64_t)(unsafe.Pointer(&ids[0])), C.int64_t(n),
		&cnt) != C.PCGX_OK {
		return []int{}
	}
	return idsToInt(ids[:int(cnt)])
}

// SegmentByID returns the same set in ascending id order from region labels of the whole cloud
// (computed once per maxRange): the fast path for many seeds.
func (r *RegionGrowing) SegmentByID(p mat.Vec3, maxRange float32) []int {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(r) // the finalizer must not free the handle while a call is in flight
	n := len(r.labels)
	if n == 0 {
		return []int{}
	}
	if r.comp == nil || r.maxRange != maxRange {
		comp := make([]int64, n)
		if C.pcgx_region_growing_components(r.search.t.h, (*C.uint32_t)(unsafe.Pointer(&r.labels[0])), C.float(maxRange),
			(*C.int64_t)(unsafe.Pointer(&comp[0]))) != C.PCGX_OK {
			return []int{}
		}
		r.comp, r.maxRange = comp, maxRange
	}
	ids := make([]int64, n)
	var cnt C.int64_t
	if C.pcgx_region_growing_segment(r.search.t.h, (*C.uint32_t)(unsafe.Pointer(&r.labels[0])),
		(*C.int64_t)(unsafe.Pointer(&r.comp[0])), (*C.float)(unsafe.Pointer(&p[0])), C.float(maxRange),
		(*C.int64_t)(unsafe.Pointer(&ids[0])), C.int64_t(n), &cnt) != C.PCGX_OK {
		return []int{}
	}
	return idsToInt(ids[:int(cnt)])
}


// ------------------------------------------ strict sums and the sharded Fit

// FitStrict is Fit with Evaluator.Sums forced to SumsReference, whatever e.Sums says: the evaluator's
// sums formed exactly as the Go code forms them (sequential float32 additions in target order,
// evaluator.go:122-145), so the returned transform and Stat are bit-identical to
// PointToPointICPGradient.Fit on the CPU at any size.  Since SumsReference is the zero value, Fit
// already does this for an Evaluator that does not ask for anything else; the name is kept for callers
// written against the earlier shim, where the float64 reduction was the default.
func FitStrict(base *KDTree, target pc.Vec3RandomAccessor, e *Evaluator, u *icp.GradientDescentUpdaterFactory) (mat.Mat4, icp.Stat, error) {
	strict := *e
	strict.Sums = SumsReference
	return Fit(base, target, &strict, u)
}

// Comm is the exchange of the sharded Fit: one process per GPU, every rank with a replica of the
// base tree and one spatial tile of the target; per iteration the ten float64 partial sums are
// all-reduced over the ranks (RCCL over xGMI, bound by libpcgx.so at run time).
type Comm struct{ h *C.pcgx_comm }

// CommID is generated by rank 0 (NewCommID) and handed to every rank by any channel the host has.
type CommID [128]byte

func NewCommID() (CommID, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var id CommID
	err := status(C.pcgx_comm_unique_id((*C.pcgx_comm_id)(unsafe.Pointer(&id[0]))))
	return id, err
}

// NewComm is collective: every rank calls it with the same id.
func NewComm(rank, world int, id CommID) (*Comm, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	c := &Comm{}
	if err := status(C.pcgx_comm_init(C.int32_t(rank), C.int32_t(world), (*C.pcgx_comm_id)(unsafe.Pointer(&id[0])), &c.h)); err != nil {
		return nil, err
	}
	return c, nil
}

func (c *Comm) Close() {
	if c.h != nil {
		C.pcgx_comm_free(c.h)
		c.h = nil
	}
}

// InitDevices: one process drives several GPUs (SURVEY 8(b): the reference is one process, icp.go:23).  Slot k of
// the library works on HIP device ids[k] (nil: device k).  A goroutine names the slot its calls are for with
// SetDevice -- after runtime.LockOSThread: the slot is per OS thread, like HIP's current device -- and a tree
// belongs to the slot it was built on.  FitMulti needs none of that from the caller.
func InitDevices(n int, ids []int32) error {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var p *C.int32_t
	if len(ids) > 0 {
		p = (*C.int32_t)(unsafe.Pointer(&ids[0]))
	}
	return status(C.pcgx_init_devices(C.int32_t(n), p))
}

// SetDevice selects the calling OS thread's device slot (call runtime.LockOSThread first).
func SetDevice(slot int) error { return status(C.pcgx_set_device(C.int32_t(slot))) }

// NewReplicas builds the same tree on the first n device slots (one upload and build per slot).
func NewReplicas(ra pc.Vec3RandomAccessor, n int, opts ...KDTreeOption) ([]*KDTree, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer C.pcgx_set_device(0)
	out := make([]*KDTree, 0, n)
	for r := 0; r < n; r++ {
		if err := SetDevice(r); err != nil {
			return nil, err
		}
		k, err := New(ra, opts...)
		if err != nil {
			return nil, err
		}
		out = append(out, k)
	}
	return out, nil
}

// FitMulti is Fit with the target spread over the device slots of THIS process: bases[r] is the replica on slot r
// (NewReplicas), tiles[r] slot r's part of the target.  With the default sums (e.Sums == 0) the result is the
// reference's Fit of the tiles one after the other, bit for bit (icp.go:23-67, evaluator.go:122-145); no second
// process, no communicator to set up.  A slot whose step fails ends the Fit on every slot (the error names it).
func FitMulti(bases []*KDTree, tiles []pc.Vec3RandomAccessor, e *Evaluator, u *icp.GradientDescentUpdaterFactory) (mat.Mat4, icp.Stat, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	n := len(bases)
	if n == 0 || len(tiles) != n {
		return mat.Mat4{}, icp.Stat{}, errors.New("pcgx: FitMulti needs one tile per base replica")
	}
	var p C.pcgx_icp_params
	p.max_dist, p.min_dist_sq, p.min_pairs = C.float(e.MaxDist), C.float(bases[0].MinDistSq), C.int32_t(e.MinPairs)
	p.weight_fn, p.weight_fn_param = C.int32_t(e.Weight.Kind), C.float(e.Weight.A)
	p.sums_mode = C.int32_t(e.Sums)
	if u != nil {
		for i := 0; i < 6; i++ {
			p.weight[i], p.threshold[i] = C.float(u.Weight[i]), C.float(u.Threshold[i])
		}
		p.max_iteration = C.int32_t(u.MaxIteration)
	}
	// the C side reads the arrays of pointers during the call only; they live in C memory (cgo: no Go pointers to Go pointers)
	hb := (*[1 << 20]*C.pcgx_kdtree)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))
	ht := (*[1 << 20]*C.float)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))
	hn := (*[1 << 20]C.int64_t)(C.malloc(C.size_t(n) * 8))
	defer C.free(unsafe.Pointer(hb))
	defer C.free(unsafe.Pointer(ht))
	defer C.free(unsafe.Pointer(hn))
	packed := make([][]float32, n)
	var pin runtime.Pinner // the tiles' memory is referenced from C memory for the length of the call
	defer pin.Unpin()
	for r := 0; r < n; r++ {
		packed[r] = packVec3(tiles[r])
		hb[r] = bases[r].t.h
		hn[r] = C.int64_t(tiles[r].Len())
		ht[r] = nil
		if len(packed[r]) > 0 {
			pin.Pin(&packed[r][0])
			ht[r] = (*C.float)(unsafe.Pointer(&packed[r][0]))
		}
	}
	var trans mat.Mat4
	var st C.pcgx_icp_stat
	rc := C.pcgx_icp_fit_multi(C.int32_t(n), (**C.pcgx_kdtree)(unsafe.Pointer(hb)), (**C.float)(unsafe.Pointer(ht)),
		(*C.int64_t)(unsafe.Pointer(hn)), &p, (*C.float)(unsafe.Pointer(&trans[0])), &st)
	runtime.KeepAlive(bases)
	runtime.KeepAlive(packed)
	stat := icp.Stat{NumIteration: int(st.num_iteration)}
	stat.Value, stat.DistRMS = float32(st.evaluated.value), float32(st.evaluated.dist_rms)
	for i := 0; i < 6; i++ {
		stat.Gradient[i] = float32(st.evaluated.gradient[i])
	}
	return trans, stat, status(rc)
}

// FitSharded runs Fit on this rank's tile of the target; every rank returns the same transform.
// With the default sums (e.Sums == 0) that is the reference's Fit of the ranks' tiles one after the other, rank 0's
// first, bit for bit (its sequential float32 sums go round the ranks); SumsF64Tree is one all-reduce of ten float64
// per iteration.  A communicator of one rank is Fit.
func FitSharded(base *KDTree, tile pc.Vec3RandomAccessor, e *Evaluator, u *icp.GradientDescentUpdaterFactory, c *Comm) (mat.Mat4, icp.Stat, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(base)
	defer runtime.KeepAlive(c)
	var p C.pcgx_icp_params
	p.max_dist, p.min_dist_sq, p.min_pairs = C.float(e.MaxDist), C.float(base.MinDistSq), C.int32_t(e.MinPairs)
	p.weight_fn, p.weight_fn_param = C.int32_t(e.Weight.Kind), C.float(e.Weight.A)
	p.sums_mode = C.int32_t(e.Sums)
	if u != nil {
		for i := 0; i < 6; i++ {
			p.weight[i], p.threshold[i] = C.float(u.Weight[i]), C.float(u.Threshold[i])
		}
		p.max_iteration = C.int32_t(u.MaxIteration)
	}
	t := packVec3(tile)
	var tp *C.float
	if len(t) > 0 {
		tp = (*C.float)(unsafe.Pointer(&t[0]))
	}
	var trans mat.Mat4
	var st C.pcgx_icp_stat
	rc := C.pcgx_icp_fit_sharded(base.t.h, tp, C.int64_t(tile.Len()), &p, c.h, (*C.float)(unsafe.Pointer(&trans[0])), &st)
	stat := icp.Stat{NumIteration: int(st.num_iteration)}
	stat.Value, stat.DistRMS = float32(st.evaluated.value), float32(st.evaluated.dist_rms)
	for i := 0; i < 6; i++ {
		stat.Gradient[i] = float32(st.evaluated.gradient[i])
	}
	return trans, stat, status(rc)
}

// ------------------------------------------------- sample consensus plane detection

// SACPlane is voxelGridSurfaceModelCoefficients (pc/sac/surface.go:191-200); its layout is pcgx_sac_plane's.
type SACPlane struct {
	Origin, V1, V2 mat.Vec3
	L1, L2         float32
	Norm           mat.Vec3
	D              float32
}

func (c *SACPlane) cptr() *C.pcgx_sac_plane { return (*C.pcgx_sac_plane)(unsafe.Pointer(c)) }

// SACPlaneModel is pc/sac's voxelGridSurfaceModel (surface.go:9-34) on the device: the cloud's xyz, the grid's
// occupied voxels and bucket lengths, vg.MinMax() and Resolution() copied at creation.
type SACPlaneModel struct {
	h *C.pcgx_sac_plane_model
	n int
}

// NewSACPlaneModel copies ra and the buckets of g into library-owned device memory.
func NewSACPlaneModel(g *BucketGrid, ra pc.Vec3RandomAccessor) (*SACPlaneModel, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(g)
	xyz := packVec3(ra)
	var data unsafe.Pointer
	if len(xyz) > 0 {
		data = unsafe.Pointer(&xyz[0])
	}
	m := &SACPlaneModel{n: ra.Len()}
	rc := C.pcgx_sac_plane_model_create(g.h, data, C.int64_t(ra.Len()), 12, 0, 0, &m.h)
	runtime.KeepAlive(xyz)
	if err := status(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(m, func(m *SACPlaneModel) { m.Close() })
	return m, nil
}

// Close releases the model.
func (m *SACPlaneModel) Close() {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(m)
	if m.h != nil {
		C.pcgx_sac_plane_model_free(m.h)
		m.h = nil
	}
}

// Len is ra.Len() of the model's cloud.
func (m *SACPlaneModel) Len() int { return m.n }

// SACResult is one Compute over pre-drawn ids: the first hypothesis of the largest score above 0 (sac.go:49),
// and every hypothesis' Fit flag, coefficients and Evaluate().
type SACResult struct {
	Found     bool
	Best      int
	BestScore int
	BestCoeff SACPlane
	OK        []bool
	Coeff     []SACPlane
	Score     []int
}

// Compute fits and evaluates len(ids)/3 hypotheses in one device call.  An id outside [0, Len()) is
// ErrOutOfRange (the reference panics).
func (m *SACPlaneModel) Compute(ids []int) (*SACResult, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(m)
	if len(ids)%3 != 0 {
		return nil, errors.New("pcgx: three ids per hypothesis")
	}
	n := len(ids) / 3
	ids64 := make([]int64, len(ids)+1)
	for i, v := range ids {
		ids64[i] = int64(v)
	}
	ok := make([]int32, n+1)
	coeff := make([]SACPlane, n+1)
	score := make([]int64, n+1)
	var found C.int32_t
	var best, bestScore C.int64_t
	r := &SACResult{}
	rc := C.pcgx_sac_plane_compute(m.h, (*C.int64_t)(unsafe.Pointer(&ids64[0])), C.int64_t(n), &found, &best, &bestScore,
		r.BestCoeff.cptr(), (*C.int32_t)(unsafe.Pointer(&ok[0])), coeff[0].cptr(), (*C.int64_t)(unsafe.Pointer(&score[0])))
	runtime.KeepAlive(ids64)
	runtime.KeepAlive(ok)
	runtime.KeepAlive(coeff)
	runtime.KeepAlive(score)
	if err := status(rc); err != nil {
		return nil, err
	}
	r.Found, r.Best, r.BestScore = found != 0, int(best), int(bestScore)
	r.OK = make([]bool, n)
	r.Score = make([]int, n)
	for i := 0; i < n; i++ {
		r.OK[i] = ok[i] != 0
		r.Score[i] = int(score[i])
	}
	r.Coeff = coeff[:n]
	return r, nil
}

// Inliers is Inliers(d) (surface.go:222-235) of c over the model's cloud, ids ascending.
func (m *SACPlaneModel) Inliers(c *SACPlane, d float32) []int {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(m)
	var cnt C.int64_t
	if C.pcgx_sac_plane_inliers(m.h, c.cptr(), C.float(d), nil, 0, &cnt) != C.PCGX_OK || cnt <= 0 {
		return []int{}
	}
	ids := make([]int64, int(cnt))
	C.pcgx_sac_plane_inliers(m.h, c.cptr(), C.float(d), (*C.int64_t)(unsafe.Pointer(&ids[0])), cnt, &cnt)
	runtime.KeepAlive(ids)
	return idsToInt(ids[:int(cnt)])
}

// IsIn is IsIn(p, d) (surface.go:237-240).
func (m *SACPlaneModel) IsIn(c *SACPlane, p mat.Vec3, d float32) bool {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(m)
	var in C.int32_t
	C.pcgx_sac_plane_is_in(m.h, c.cptr(), (*C.float)(unsafe.Pointer(&p[0])), C.float(d), &in)
	return in != 0
}

// ------------------------------------------------- NDT registration (extension: no reference parity)

// NDTMap is the base cloud as one Gaussian per occupied voxel of a BucketGrid (include/pcgx.h, "Normal Distributions
// Transform").  No counterpart in the reference.  The map copies what it needs: the grid and the cloud may go afterwards.
type NDTMap struct {
	h *C.pcgx_ndt_map
}

// NDTCells lists the occupied voxels in ascending address; Cov and ICov are xx, xy, xz, yy, yz, zz, zero when invalid.
type NDTCells struct {
	Addr  []int64
	Count []int32
	Valid []int32
	Mean  []mat.Vec3
	Cov   [][6]float32
	ICov  [][6]float32
}

// NewNDTMap builds the map over ra, the cloud g was built from.  A voxel with fewer than max(minPoints, 3) points, or
// whose points coincide, is invalid; a valid voxel's eigenvalues are raised to minEigenRatio times the largest.
func NewNDTMap(g *BucketGrid, ra pc.Vec3RandomAccessor, minPoints int, minEigenRatio float32) (*NDTMap, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(g)
	xyz := packVec3(ra)
	var data unsafe.Pointer
	if len(xyz) > 0 {
		data = unsafe.Pointer(&xyz[0])
	}
	m := &NDTMap{}
	rc := C.pcgx_ndt_map_create(g.h, data, C.int64_t(ra.Len()), 12, 0, 0, C.int32_t(minPoints), C.float(minEigenRatio), &m.h)
	runtime.KeepAlive(xyz)
	if err := status(rc); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(m, func(m *NDTMap) { m.Close() })
	return m, nil
}

// Close releases the map.
func (m *NDTMap) Close() {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(m)
	if m.h != nil {
		C.pcgx_ndt_map_free(m.h)
		m.h = nil
	}
}

// Counts returns the numbers of occupied and of valid voxels.
func (m *NDTMap) Counts() (occupied, valid int, err error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(m)
	var a, b C.int64_t
	err = status(C.pcgx_ndt_map_counts(m.h, &a, &b))
	return int(a), int(b), err
}

// Cells reads the map out.
func (m *NDTMap) Cells() (*NDTCells, error) {
	n, _, err := m.Counts()
	if err != nil {
		return nil, err
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(m)
	c := &NDTCells{Addr: make([]int64, n), Count: make([]int32, n), Valid: make([]int32, n), Mean: make([]mat.Vec3, n),
		Cov: make([][6]float32, n), ICov: make([][6]float32, n)}
	if n == 0 {
		return c, nil
	}
	rc := C.pcgx_ndt_map_cells(m.h, (*C.int64_t)(unsafe.Pointer(&c.Addr[0])), (*C.int32_t)(unsafe.Pointer(&c.Count[0])),
		(*C.int32_t)(unsafe.Pointer(&c.Valid[0])), (*C.float)(unsafe.Pointer(&c.Mean[0][0])),
		(*C.float)(unsafe.Pointer(&c.Cov[0][0])), (*C.float)(unsafe.Pointer(&c.ICov[0][0])))
	return c, status(rc)
}

// Evaluate returns the 30 float64 sums {sum e, sum g [6], upper triangle of sum H [21], sum omega, pair count} of the
// target at pose trans (nil: the identity); neighbors is 1, 7 or 27.
func (m *NDTMap) Evaluate(target pc.Vec3RandomAccessor, trans *mat.Mat4, neighbors int, outlierRatio float32) ([30]float64, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(m)
	var sums [30]float64
	t := packVec3(target)
	var tp, pose *C.float
	if len(t) > 0 {
		tp = (*C.float)(unsafe.Pointer(&t[0]))
	}
	if trans != nil {
		pose = (*C.float)(unsafe.Pointer(&trans[0]))
	}
	rc := C.pcgx_ndt_evaluate(m.h, tp, C.int64_t(target.Len()), pose, C.int32_t(neighbors), C.float(outlierRatio),
		(*C.double)(unsafe.Pointer(&sums[0])))
	return sums, status(rc)
}

// NDT is the Fit on an NDTMap: evaluate, the plane Fit's evaluate tail, the Gauss-Newton update, repeated on the device
// with one read-back.  Zero values select the defaults of the plane Fit (MinPairs 6, Threshold 0.01, MaxIteration 20);
// Neighbors 0 selects 7 and OutlierRatio 0 selects 0.55.
type NDT struct {
	Neighbors    int
	OutlierRatio float32
	MinPairs     int
	Threshold    mat.Vec6
	MaxIteration int
	Damping      float32
}

// Fit moves target onto the map, starting from init (nil: the identity).  When no point sees a valid voxel with a
// weight above zero the gradient is 0 and init comes back as converged: Evaluate's sums[28] (sum omega) tells.
func (n *NDT) Fit(m *NDTMap, target pc.Vec3RandomAccessor, init *mat.Mat4) (mat.Mat4, icp.Stat, error) {
	runtime.LockOSThread() // the error text is thread-local on the C side: call and pcgx_last_error on one OS thread
	defer runtime.UnlockOSThread()
	defer runtime.KeepAlive(m)
	var trans mat.Mat4
	stat := icp.Stat{}
	var p C.pcgx_icp_params
	p.min_pairs, p.max_iteration = C.int32_t(n.MinPairs), C.int32_t(n.MaxIteration)
	for i := 0; i < 6; i++ {
		p.threshold[i] = C.float(n.Threshold[i])
	}
	nb, outlier := n.Neighbors, n.OutlierRatio
	if nb == 0 {
		nb = 7
	}
	if outlier == 0 {
		outlier = 0.55
	}
	t := packVec3(target)
	var tp, ip *C.float
	if len(t) > 0 {
		tp = (*C.float)(unsafe.Pointer(&t[0]))
	}
	if init != nil {
		ip = (*C.float)(unsafe.Pointer(&init[0]))
	}
	var st C.pcgx_icp_stat
	rc := C.pcgx_ndt_fit(m.h, tp, C.int64_t(target.Len()), 0, &p, C.float(n.Damping), C.int32_t(nb), C.float(outlier), ip,
		(*C.float)(unsafe.Pointer(&trans[0])), &st, (*C.float)(unsafe.Pointer(&stat.Hessian[0])))
	return trans, stat, gicpStat(&st, &stat, rc)
}
