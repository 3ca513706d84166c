// Package sac is the GPU drop-in for github.com/seqsense/pcgol/pc/sac: the same exported names (sac.go:7-63,
// randomsample.go:7-12, surface.go:20-34), with the model over a device bucket grid (pcgx.BucketGrid).
// Compute(n) draws the 3n ids from s.Sampler first, in the reference's order (sac.go:40-43), then fits and
// evaluates every hypothesis in ONE device call: neither Fit nor Evaluate draws random numbers, so the result is
// the reference loop's for the same draws.
//
// NOT compiled in the build image (no Go toolchain there); see go/README.md.
package sac

import (
	"math/rand"

	"github.com/seqsense/pcgol/mat"
	"github.com/seqsense/pcgol/pc"

	"github.com/seqsense/pcgol/gpu/pcgx"
)

type Sampler interface {
	Sample() int
}

type Model interface {
	NumRange() (min, max int)
	Fit([]int) (ModelCoefficients, bool)
}

type ModelCoefficients interface {
	Evaluate() int
	Inliers(float32) []int
	IsIn(mat.Vec3, float32) bool
}

// batchModel is what Compute needs to fit and evaluate many hypotheses in one call.
type batchModel interface {
	computeBatch(ids []int) (ModelCoefficients, bool)
}

type SAC struct {
	Sampler Sampler
	Model   Model

	bestCoeff ModelCoefficients
}

func New(s Sampler, m Model) *SAC {
	return &SAC{Sampler: s, Model: m}
}

// Compute is sac.go:33-59.  A Model other than this package's runs the reference's loop.
func (s *SAC) Compute(n int) bool {
	num, _ := s.Model.NumRange()
	bm, batched := s.Model.(batchModel)
	if !batched {
		var bestCoeff ModelCoefficients
		var bestE int
		ids := make([]int, num)
		for i := 0; i < n; i++ {
			for j := 0; j < num; j++ {
				ids[j] = s.Sampler.Sample()
			}
			coeff, ok := s.Model.Fit(ids)
			if !ok {
				continue
			}
			if e := coeff.Evaluate(); e > bestE {
				bestE, bestCoeff = e, coeff
			}
		}
		if bestCoeff == nil {
			return false
		}
		s.bestCoeff = bestCoeff
		return true
	}
	if n <= 0 {
		return false
	}
	ids := make([]int, 0, n*num)
	for i := 0; i < n*num; i++ {
		ids = append(ids, s.Sampler.Sample())
	}
	best, ok := bm.computeBatch(ids)
	if !ok {
		return false
	}
	s.bestCoeff = best
	return true
}

func (s *SAC) Coefficients() ModelCoefficients {
	return s.bestCoeff
}

// NewRandomSampler is randomsample.go:7-12 (Go's math/rand, as the reference).
func NewRandomSampler(n int) Sampler {
	if n < 0x8000000 {
		return &randomSampler31{int32(n)}
	}
	return &randomSampler63{int64(n)}
}

type randomSampler31 struct{ n int32 }

func (s *randomSampler31) Sample() int { return int(rand.Int31n(s.n)) }

type randomSampler63 struct{ n int64 }

func (s *randomSampler63) Sample() int { return int(rand.Int63n(s.n)) }

type voxelGridSurfaceModel struct {
	m *pcgx.SACPlaneModel
}

// NewVoxelGridSurfaceModel is surface.go:20-30 over a device bucket grid; the model copies vg's buckets and ra.
// It panics where the reference would (an unusable grid or cloud is a programming error there too).
func NewVoxelGridSurfaceModel(vg *pcgx.BucketGrid, ra pc.Vec3RandomAccessor) *voxelGridSurfaceModel {
	m, err := pcgx.NewSACPlaneModel(vg, ra)
	if err != nil {
		panic(err)
	}
	return &voxelGridSurfaceModel{m: m}
}

func (voxelGridSurfaceModel) NumRange() (min, max int) {
	return 3, 3
}

// Fit is surface.go:36-181 (with Evaluate computed in the same device call).
func (m *voxelGridSurfaceModel) Fit(ids []int) (ModelCoefficients, bool) {
	if len(ids) != 3 {
		return nil, false
	}
	r, err := m.m.Compute(ids)
	if err != nil {
		panic(err) // an id outside the cloud: the reference panics (index out of range)
	}
	if !r.OK[0] {
		return nil, false
	}
	return &coefficients{model: m, c: r.Coeff[0], score: r.Score[0]}, true
}

func (m *voxelGridSurfaceModel) computeBatch(ids []int) (ModelCoefficients, bool) {
	r, err := m.m.Compute(ids)
	if err != nil {
		panic(err)
	}
	if !r.Found {
		return nil, false
	}
	return &coefficients{model: m, c: r.BestCoeff, score: r.BestScore}, true
}

type coefficients struct {
	model *voxelGridSurfaceModel
	c     pcgx.SACPlane
	score int
}

func (c *coefficients) Evaluate() int                   { return c.score }
func (c *coefficients) Inliers(d float32) []int         { return c.model.m.Inliers(&c.c, d) }
func (c *coefficients) IsIn(p mat.Vec3, d float32) bool { return c.model.m.IsIn(&c.c, p, d) }
