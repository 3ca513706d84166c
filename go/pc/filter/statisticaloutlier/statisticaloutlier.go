// Package statisticaloutlier is statistical outlier removal behind filter.Filter (pc/filter/filter.go:7-9), in the
// option style of pc/filter/voxelgrid (option.go:7-18).  No counterpart in the reference (PCL's
// StatisticalOutlierRemoval): every call is answered by libpcgx.so (include/pcgx.h, pcgx_sor_filter) through the cgo
// package ../../../pcgx.
//
// NOT compiled in the build image (no Go toolchain there); see go/README.md.
package statisticaloutlier

import (
	"github.com/seqsense/pcgol/pc/filter"

	"github.com/seqsense/pcgol/gpu/pcgx"
)

// Options of the filter.
type Options struct {
	MeanK     int     // neighbours a point's mean distance is taken over, 1..64
	StddevMul float32 // the threshold is mu + StddevMul * sigma of the mean distances
	Negative  bool    // keep the outliers instead
}

// Option sets one of Options.
type Option func(*Options)

// WithNegative keeps the points the filter would remove (among the finite ones) instead.
func WithNegative(negative bool) Option {
	return Option(func(o *Options) {
		o.Negative = negative
	})
}

// New returns the filter: Filter(pp) keeps the points whose mean distance to their meanK nearest other finite
// points is at most mu + stddevMul * sigma, records byte for byte in input order (Width = M, Height = 1).
func New(meanK int, stddevMul float32, opts ...Option) filter.Filter {
	o := Options{MeanK: meanK, StddevMul: stddevMul}
	for _, f := range opts {
		f(&o)
	}
	return &pcgx.SOR{MeanK: o.MeanK, StddevMul: o.StddevMul, Negative: o.Negative}
}
