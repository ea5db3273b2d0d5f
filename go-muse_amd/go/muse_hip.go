// Package muse -- cgo binding of libmuse_hip.so for aouyang1/go-muse.
//
// WRITTEN BLIND: the build image has no Go toolchain, so this file has never
// been compiled.  It is the reference-side binding a maintainer would add next
// to the existing sources (series.go, group.go, labels.go, results.go,
// scores.go stay as they are); it replaces the bodies of NewBatch / Batch.Run
// (muse_batch.go:23-130) and New / Muse.Run (muse.go:23-92) and deletes
// xcorr.go's hot loop.  Every cgo call copies its inputs (no Go pointer is
// retained by C after the call returns), as the cgo pointer rules require.
//
// Builds at the reference's own language level (go.mod:3, go 1.13): C memory is viewed through the array-pointer
// idiom (f64View ... below), not unsafe.Slice / unsafe.Add (Go 1.17).
// Build: CGO_CFLAGS="-I${REPO}/include" CGO_LDFLAGS="-L${REPO}/go-muse_amd/lib -lmuse_hip"
package muse

/*
#cgo LDFLAGS: -lmuse_hip
#include <stdlib.h>
#include "muse_hip.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"sort"
	"sync"
	"sync/atomic"
	"unsafe"
)

// Views of C memory as Go slices (n <= maxView elements; the array types only bound the index arithmetic, nothing of
// that size is ever allocated).
const maxView = 1 << 30

func f64View(p unsafe.Pointer, n int) []float64 { return (*[maxView]float64)(p)[:n:n] }
func i32View(p unsafe.Pointer, n int) []int32   { return (*[maxView]int32)(p)[:n:n] }
func u8View(p *C.uint8_t, n int) []C.uint8_t    { return (*[maxView]C.uint8_t)(unsafe.Pointer(p))[:n:n] }
func recView(p *C.muse_record, n int) []C.muse_record {
	return (*[maxView]C.muse_record)(unsafe.Pointer(p))[:n:n]
}
func batchView(p **C.muse_batch, n int) []*C.muse_batch {
	return (*[maxView]*C.muse_batch)(unsafe.Pointer(p))[:n:n]
}

// hipError turns a muse_status into a Go error carrying muse_last_error().
func hipError(status C.int) error {
	if status == C.MUSE_OK {
		return nil
	}
	return errors.New(C.GoString(C.muse_last_error()))
}

// engine is one muse_ctx (one GPU).  A process-wide default is created lazily.
type engine struct{ ctx *C.muse_ctx }

var (
	defaultEngine    *engine
	defaultEngineErr error
	defaultEngineOne sync.Once
)

// getEngine creates the process-wide context exactly once, however many goroutines race to the first
// use (muse_test.go:203-214 drives one Muse from many goroutines).  A failed creation is remembered:
// there is no CPU fallback to retry into.
func getEngine() (*engine, error) {
	// SetDevices([]int{k}): ONE engine selected -- every unsharded path (Batch, Muse, xCorr) runs on that device, as the
	// Python and C++ mirrors do with engines[0]; the default context on device 0 is not created for it
	engineSetMu.Lock()
	if len(engineSet) == 1 {
		e := engineSet[0]
		engineSetMu.Unlock()
		return e, nil
	}
	engineSetMu.Unlock()
	defaultEngineOne.Do(func() {
		e := &engine{}
		// a cgo call and the muse_last_error that explains it must run on one OS thread
		runtime.LockOSThread()
		defer runtime.UnlockOSThread()
		if err := hipError(C.muse_ctx_create(0, &e.ctx)); err != nil {
			defaultEngineErr = err
			return
		}
		defaultEngine = e
	})
	return defaultEngine, defaultEngineErr
}

// The device set a Batch shards its Comparison group over (SURVEY 8e: the goroutine fan-out of
// muse_batch.go:99-130 becomes one goroutine per GPU, each driving its own muse_ctx).  Default: device 0 only.
var (
	engineSet   []*engine
	engineSetMu sync.Mutex
)

// SetDevices selects the GPUs every later Batch.Run shards over (one muse_ctx per listed device; a device may be
// listed more than once).  A single id selects that device for the unsharded path.  SetDevices(nil) goes back to the
// single default engine (device 0).  DeviceCount() tells how many
// the process can see; SetDevices(AllDevices()) is the eight-GPU configuration of one node.
func SetDevices(ids []int) error {
	engineSetMu.Lock()
	defer engineSetMu.Unlock()
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var set []*engine
	for _, id := range ids {
		e := &engine{}
		if err := hipError(C.muse_ctx_create(C.int32_t(id), &e.ctx)); err != nil {
			for _, d := range set {
				C.muse_ctx_destroy(d.ctx)
			}
			return err
		}
		set = append(set, e)
	}
	for _, d := range engineSet {
		C.muse_ctx_destroy(d.ctx) // (reference-counted: lives until its last group / batch is freed)
	}
	engineSet = set
	return nil
}

// DeviceCount returns the number of gfx950 devices visible to the process.
func DeviceCount() (int, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var n C.int32_t
	if err := hipError(C.muse_device_count(&n)); err != nil {
		return 0, err
	}
	return int(n), nil
}

// AllDevices lists every visible device once.
func AllDevices() []int {
	n, _ := DeviceCount()
	ids := make([]int, n)
	for i := range ids {
		ids[i] = i
	}
	return ids
}

func shardEngines() []*engine {
	engineSetMu.Lock()
	defer engineSetMu.Unlock()
	if len(engineSet) < 2 {
		return nil
	}
	return append([]*engine(nil), engineSet...)
}

// SetScreening switches the filter-and-refine Run of the default engine (include/muse_hip.h:
// muse_ctx_set_screening; OFF by default -- every series is scored in float64 like the reference --;
// when on, Runs over large groups screen every series in fp32 and re-evaluate in fp64 only the rows that
// can reach the top-N: same Scores).
// minRows > 1 sets the smallest group the path is used for.
func SetScreening(enable bool, minRows int) error {
	e, err := getEngine()
	if err != nil {
		return err
	}
	v := C.int32_t(0)
	if enable {
		v = 1
		if minRows > 1 {
			v = C.int32_t(minRows)
		}
	}
	return hipError(C.muse_ctx_set_screening(e.ctx, v))
}

// SetSpectrumCache switches the spectrum cache of the default engine (include/muse_hip.h: muse_ctx_set_spectrum_cache; ON by
// default): a float64 group of at least 65 536 series of length 2049 .. 4096 that is scored a second time keeps the forward
// spectra of its rows in HBM (its footprint doubles, if that fits in half of the free memory) and every later Run reads them
// instead of the rows: same Scores, about half the arithmetic.
func SetSpectrumCache(on bool) error {
	e, err := getEngine()
	if err != nil {
		return err
	}
	v := C.int32_t(0)
	if on {
		v = 1
	}
	return hipError(C.muse_ctx_set_spectrum_cache(e.ctx, v))
}

// appendSeries uploads series (all of length n) to a device group through the library's pinned staging windows
// (muse_group_stage / muse_group_commit): every Series is copied ONCE, straight out of its Go slice into pinned C memory, by a
// few goroutines in pieces of ~256 KB; a piece that completes the packed prefix of the window commits that prefix -- runs of
// >= 4 MB, one host-to-device copy command each (a command costs ~13 us whatever its size) -- so the rows cross PCIe while the
// next pieces are packed.  No Go pointer crosses: the window is C memory, the goroutines write into it through f64View.
func appendSeries(g *C.muse_group, series []*Series, n int) error {
	for first := 0; first < len(series); {
		var win *C.double
		var granted C.int64_t
		if err := hipError(C.muse_group_stage(g, C.int64_t(len(series)-first), &win, &granted)); err != nil {
			return err
		}
		k := int(granted)
		rows := f64View(unsafe.Pointer(win), k*n)
		piece := (256 << 10) / (8 * n)
		if piece < 1 {
			piece = 1
		}
		npieces := (k + piece - 1) / piece
		commitPieces := (4 << 20) / (piece * 8 * n)
		if commitPieces < 1 {
			commitPieces = 1
		}
		workers := runtime.GOMAXPROCS(0)
		if workers > 8 {
			workers = 8
		}
		if workers > npieces {
			workers = npieces
		}
		var (
			mu        sync.Mutex
			done      = make([]bool, npieces)
			watermark = 0
			next      int64 = -1
			firstErr  error
			wg        sync.WaitGroup
		)
		for w := 0; w < workers; w++ {
			wg.Add(1)
			go func() {
				defer wg.Done()
				runtime.LockOSThread() // (muse_last_error is per host thread)
				defer runtime.UnlockOSThread()
				for {
					p := int(atomic.AddInt64(&next, 1))
					if p >= npieces {
						return
					}
					lo, hi := p*piece, (p+1)*piece
					if hi > k {
						hi = k
					}
					for r := lo; r < hi; r++ {
						copy(rows[r*n:(r+1)*n], series[first+r].y)
					}
					mu.Lock()
					done[p] = true
					wm := watermark
					for wm < npieces && done[wm] {
						wm++
					}
					if wm > watermark && (wm == npieces || wm-watermark >= commitPieces) {
						clo, chi := watermark*piece, wm*piece
						if chi > k {
							chi = k
						}
						// (every row is committed even after a failure: the window has to close)
						if err := hipError(C.muse_group_commit(g, C.int64_t(clo), C.int64_t(chi-clo))); err != nil && firstErr == nil {
							firstErr = err
						}
						watermark = wm
					}
					mu.Unlock()
				}
			}()
		}
		wg.Wait()
		if firstErr != nil {
			return firstErr
		}
		first += k
	}
	return nil
}

// deviceGroup mirrors Group's rows on the GPU; rows are appended once.
type deviceGroup struct {
	g        *C.muse_group
	uploaded int
}

// residentRows uploads the series added since the last call (Group.Add order).
// Group gains two fields: order []*Series (insertion order) and dev *deviceGroup.
func (g *Group) residentRows(e *engine) (*C.muse_group, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if g.dev == nil {
		d := &deviceGroup{}
		n := g.n
		if n < 1 {
			n = 1
		}
		if err := hipError(C.muse_group_create(e.ctx, C.int64_t(len(g.order)), C.int32_t(n), &d.g)); err != nil {
			return nil, err
		}
		runtime.SetFinalizer(d, func(d *deviceGroup) { C.muse_group_free(d.g) })
		g.dev = d
	}
	if g.dev.uploaded < len(g.order) {
		if err := appendSeries(g.dev.g, g.order[g.dev.uploaded:], g.n); err != nil {
			return nil, err
		}
		g.dev.uploaded = len(g.order)
	}
	return g.dev.g, nil
}

// groupShard is one contiguous row range of the Group on one device (the shard_bounds rule: equal shares rounded up to
// an even row count -- the fused kernels pack two series per pass).  The cut is made once, at the first sharded Run;
// series added later extend the last shard.  Group gains a third field: shards []*groupShard.
type groupShard struct {
	e                *engine
	g                *C.muse_group
	lo, hi, uploaded int
}

func (g *Group) residentShards(es []*engine) ([]*groupShard, error) {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	same := len(g.shards) == len(es)
	for i := 0; same && i < len(es); i++ {
		same = g.shards[i].e == es[i]
	}
	if !same {
		g.shards = nil // (the old shards' device groups are released by their finalizers)
		M, W := len(g.order), len(es)
		per := (M + W - 1) / W
		per = (per + 1) / 2 * 2
		n := g.n
		if n < 1 {
			n = 1
		}
		for r := 0; r < W; r++ {
			sh := &groupShard{e: es[r]}
			sh.lo = r * per
			if sh.lo > M {
				sh.lo = M
			}
			sh.hi = sh.lo + per
			if sh.hi > M {
				sh.hi = M
			}
			if err := hipError(C.muse_group_create(es[r].ctx, C.int64_t(sh.hi-sh.lo), C.int32_t(n), &sh.g)); err != nil {
				return nil, err
			}
			runtime.SetFinalizer(sh, func(sh *groupShard) { C.muse_group_free(sh.g) })
			g.shards = append(g.shards, sh)
		}
	}
	if len(g.shards) > 0 {
		g.shards[len(g.shards)-1].hi = len(g.order) // series added since the cut
	}
	for _, sh := range g.shards {
		if sh.lo+sh.uploaded < sh.hi {
			if err := appendSeries(sh.g, g.order[sh.lo+sh.uploaded:sh.hi], g.n); err != nil {
				return nil, err
			}
			sh.uploaded = sh.hi - sh.lo
		}
	}
	return g.shards, nil
}

// Batch keeps the exported fields of muse_batch.go:13-19; x and n are gone
// (the reference spectrum lives on the device).
type Batch struct {
	ref         []float64
	Comparison  *Group
	Results     *Results
	Concurrency int
	probe       *C.muse_group // empty group the template batch is bound to
	template    *C.muse_batch // owns the reference spectrum: validated and transformed ONCE, in NewBatch
	batch       *C.muse_batch // the batch over the Comparison group's resident rows: shares the template's spectrum
	batchGroup  *C.muse_group
	shardBatch  []*C.muse_batch // sharded Runs (SetDevices): one device batch per shard
	shardGroup  []*C.muse_group
	window      int // RunWindowed: the lag window of the Run in progress (-1: none)
}

// NewBatch replaces muse_batch.go:23-52: same length check, same
// "Invalid input query" error on a constant reference.
func NewBatch(ref *Series, comp *Group, results *Results, cc int) (*Batch, error) {
	for uid, s := range comp.registry {
		if ref.Length() != s.Length() {
			return nil, fmt.Errorf("%s from comparison group series does not have the same length as the reference", uid)
		}
	}
	if cc < 1 {
		cc = 1
	}
	e, err := getEngine()
	if err != nil {
		return nil, err
	}
	b := &Batch{ref: append([]float64(nil), ref.Values()...), Comparison: comp, Results: results, Concurrency: cc, window: -1}
	// validate the reference now (sigma == 0 -> error), as the reference does
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if err := hipError(C.muse_group_create(e.ctx, 0, C.int32_t(len(b.ref)), &b.probe)); err != nil {
		return nil, err
	}
	st := C.muse_batch_create(e.ctx, b.probe, (*C.double)(unsafe.Pointer(&b.ref[0])), C.int32_t(len(b.ref)), &b.template)
	if err := hipError(st); err != nil {
		C.muse_group_free(b.probe)
		return nil, fmt.Errorf("Invalid input query, %v", err)
	}
	// the device handles are released with the Batch (muse_batch_free takes no error path)
	runtime.SetFinalizer(b, func(b *Batch) {
		if b.batch != nil {
			C.muse_batch_free(b.batch)
			b.batch = nil
		}
		C.muse_batch_free(b.template)
		C.muse_group_free(b.probe)
		for _, sb := range b.shardBatch {
			if sb != nil {
				C.muse_batch_free(sb)
			}
		}
		b.shardBatch = nil
	})
	return b, nil
}

// Run replaces muse_batch.go:99-130.  groupByLabels semantics are unchanged
// (indexLabelValues, group.go:76-104); the goroutine fan-out becomes one fused
// kernel launch over the resident matrix plus a device-side group-max / top-N.
func (b *Batch) Run(groupByLabels []string) error {
	labelValuesSet := b.Comparison.indexLabelValues(groupByLabels)
	if len(labelValuesSet) == 0 {
		return nil
	}
	// group id of every series, in upload order
	pos := make(map[string]int, len(b.Comparison.order))
	for i, s := range b.Comparison.order {
		pos[s.UID()] = i
	}
	gid := make([]C.int32_t, len(b.Comparison.order))
	gi := 0
	for _, lv := range labelValuesSet {
		for _, uid := range b.Comparison.index[lv.ID(lv.Keys())] {
			gid[pos[uid]] = C.int32_t(gi)
		}
		gi++
	}
	// Up to exactFeedMaxGroups label groups Results is fed the reference's own sequence: ONE Score per label group, in group
	// order, through the unchanged Results.Update (muse_batch.go:124-128) -- the heap's history, and with it the order Fetch
	// returns exactly tied scores in and which of them survives at the TopN boundary, also into a Results that earlier Runs
	// have filled (results.go:55-72), on one device or sharded.  Beyond it (Run(nil) over a million series) the device
	// pre-selects the TopN candidates and 24 B x TopN cross the host.
	G := len(labelValuesSet)
	exact := G <= exactFeedMaxGroups
	if es := shardEngines(); es != nil {
		return b.runSharded(es, gid, G, exact)
	}
	e, err := getEngine()
	if err != nil {
		return err
	}
	dg, err := b.Comparison.residentRows(e)
	if err != nil {
		return err
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if b.batch == nil || b.batchGroup != dg {
		if b.batch != nil {
			C.muse_batch_free(b.batch)
		}
		// (no second transform of the reference: the batch over the resident rows shares the template's spectrum)
		st := C.muse_batch_create_like(b.template, dg, &b.batch)
		if err := hipError(st); err != nil {
			return err
		}
		b.batchGroup = dg
	}
	if err := hipError(C.muse_batch_set_lag_window(b.batch, C.int32_t(b.window))); err != nil {
		return err
	}
	if exact {
		recs := (*C.muse_record)(C.calloc(C.size_t(G), C.size_t(unsafe.Sizeof(C.muse_record{}))))
		defer C.free(unsafe.Pointer(recs))
		state := (*C.uint8_t)(C.calloc(C.size_t(G), 1))
		defer C.free(unsafe.Pointer(state))
		if err := hipError(C.muse_batch_run_groups(b.batch, &gid[0], C.int32_t(G), 0, 1, recs, state)); err != nil {
			return err
		}
		return b.feedGroupWinners(recs, state, 1, G)
	}
	r := b.Results
	top := r.TopN
	if top < 1 {
		top = 1
	}
	idx := make([]C.int64_t, top)
	lag := make([]C.int32_t, top)
	score := make([]C.double, top)
	var cnt C.int32_t
	var mean C.double
	st := C.muse_batch_run(b.batch, &gid[0], C.int32_t(len(labelValuesSet)), C.int32_t(r.MaxLag), C.int32_t(r.TopN),
		C.double(r.Threshold), C.int32_t(r.SignFilter), 1, &idx[0], &lag[0], &score[0], &cnt, &mean)
	if err := hipError(st); err != nil {
		return err
	}
	// ordered drain (muse_batch.go:124-128): feed Results in group order
	order := make([]int, int(cnt))
	for i := range order {
		order[i] = i
	}
	sort.SliceStable(order, func(a, c int) bool { return gid[idx[order[a]]] < gid[idx[order[c]]] })
	for _, k := range order {
		b.Results.Update(Score{Labels: b.Comparison.order[idx[k]].Labels(), Lag: int(lag[k]), PercentScore: float64(score[k])})
	}
	return nil
}

// RunWindowed is Run with Results.MaxLag as a LAG WINDOW (muse_batch_set_lag_window): every series contributes its best
// match inside +-MaxLag, where Run drops a series whose best match over all lags lies outside.  Same feeds and devices as Run;
// the window is taken off again behind the Run, so Run itself never changes.
func (b *Batch) RunWindowed(groupByLabels []string) error {
	if b.Results.MaxLag < 0 || b.Results.MaxLag > C.MUSE_LAG_WINDOW_MAX {
		return fmt.Errorf("RunWindowed: MaxLag outside 0 .. %d", int(C.MUSE_LAG_WINDOW_MAX))
	}
	b.window = b.Results.MaxLag
	defer func() { b.window = -1 }()
	return b.Run(groupByLabels)
}

// RunInWindow is RunWindowed for ANY Results.MaxLag >= 0 (muse_batch_run_in_window): every series contributes its best match
// inside +-MaxLag -- beyond MUSE_LAG_WINDOW_MAX, and over float32-storage groups, from the transform kernels with a masked
// argmax (FFT lengths 512 ... 4096; what the library does not build comes back as its error).  One device.  Results is fed as
// Run feeds it: up to exactFeedMaxGroups label groups ONE Score per group, in group order, through Results.Update (the device
// returns every group's winner, nothing filtered but NaN, which never passes); beyond, the device's TopN pre-selection in group
// order.  The window is an argument of the call: Run and RunWindowed stay what they are.
func (b *Batch) RunInWindow(groupByLabels []string) error {
	if b.Results.MaxLag < 0 {
		return fmt.Errorf("RunInWindow: MaxLag < 0")
	}
	if es := shardEngines(); es != nil {
		return fmt.Errorf("RunInWindow runs on one device")
	}
	return b.feedInWindow(groupByLabels, false, 0, 0, false, false)
}

// RunInLagRange is RunInWindow for a one-sided or asymmetric window (muse_batch_run_in_lag_range): every series contributes its
// best match inside the lags lagLo .. lagHi, lagLo <= 0 <= lagHi (a negative lag: the series trails the reference).  One device.
// Results is fed exactly as RunInWindow feeds it; Results.Update applies the Results' own filters unchanged.
func (b *Batch) RunInLagRange(groupByLabels []string, lagLo, lagHi int) error {
	if lagLo > 0 || lagHi < 0 {
		return fmt.Errorf("RunInLagRange: lagLo <= 0 <= lagHi")
	}
	if es := shardEngines(); es != nil {
		return fmt.Errorf("RunInLagRange runs on one device")
	}
	return b.feedInWindow(groupByLabels, true, lagLo, lagHi, false, false)
}

// RunSignedInLagRange is RunInLagRange with Results.SignFilter restricting the ARGMAX, not only filtering its answer
// (muse_batch_run_signed_in_lag_range): under SignFilter_POS every series contributes its largest positive value inside the lags
// lagLo .. lagHi (SignFilter_NEG: its most negative one), so a series whose peak of the other sign is the larger one by magnitude
// is not lost, and a label group's maximum is taken over its members' values of the sign.  SignFilter_ANY is RunInLagRange.  One
// device.  Results is fed as RunInLagRange feeds it -- the sign always goes to the device, where it selects the argmax; a series
// with no value of the sign comes back as (0, +0.0), which no sign filter passes.  Under a sign the Scores carry the SIGNED value,
// clamped to +-1 as Muse.Run's are (muse.go:72-76): Batch.Run reports magnitudes (muse_batch.go:74), which SignFilter_NEG never passes.
func (b *Batch) RunSignedInLagRange(groupByLabels []string, lagLo, lagHi int) error {
	if lagLo > 0 || lagHi < 0 {
		return fmt.Errorf("RunSignedInLagRange: lagLo <= 0 <= lagHi")
	}
	if es := shardEngines(); es != nil {
		return fmt.Errorf("RunSignedInLagRange runs on one device")
	}
	return b.feedInWindow(groupByLabels, true, lagLo, lagHi, true, false)
}

// RunInLagBand is RunInLagRange for a lag band that need not hold lag 0 (muse_batch_run_in_lag_band): every series contributes its best
// match by magnitude inside the lags lagLo .. lagHi -- (1, k): the series that lead the reference by 1 .. k samples, where
// RunInLagRange(0, k) reports lag 0 for every co-moving series.  A series with nothing in the band comes back as (0, +0.0).  One
// device.  Results is fed as RunInLagRange feeds it; Results.Update applies the Results' own filters unchanged, its MaxLag included.
func (b *Batch) RunInLagBand(groupByLabels []string, lagLo, lagHi int) error {
	if lagLo > lagHi {
		return fmt.Errorf("RunInLagBand: lagLo <= lagHi")
	}
	if es := shardEngines(); es != nil {
		return fmt.Errorf("RunInLagBand runs on one device")
	}
	return b.feedInWindow(groupByLabels, true, lagLo, lagHi, false, true)
}

// RunSignedInLagBand is RunInLagBand with Results.SignFilter restricting the ARGMAX: under SignFilter_POS every series contributes its
// largest positive value inside the band, under SignFilter_NEG its most negative one; SignFilter_ANY is RunInLagBand.  Fed as
// RunSignedInLagRange feeds it: under a sign the Scores carry the signed value.
func (b *Batch) RunSignedInLagBand(groupByLabels []string, lagLo, lagHi int) error {
	if lagLo > lagHi {
		return fmt.Errorf("RunSignedInLagBand: lagLo <= lagHi")
	}
	if es := shardEngines(); es != nil {
		return fmt.Errorf("RunSignedInLagBand runs on one device")
	}
	return b.feedInWindow(groupByLabels, true, lagLo, lagHi, true, true)
}

// LagProfile returns the correlation itself at every lag of lagLo .. lagHi (muse_batch_lag_profile), where every Run returns its
// argmax alone: row k of the result, lagHi - lagLo + 1 values, is cc[(lagLo + v) mod n] of series rows[k] of the Comparison group
// (rows == nil: every series in order) -- raw values, +0.0 for a series with sigma == 0, NaN for one that holds NaN or Inf; bit for
// bit what RunInLagBand / RunInLagRange scan at that lag on the direct product.  Lags inside -(n / 2 - 1) .. n / 2, not clipped;
// float64 groups of up to 65536 samples.  One device.  The batch's scores and its window stay as they were.
func (b *Batch) LagProfile(lagLo, lagHi int, rows []int64) ([][]float64, error) {
	if lagLo > lagHi {
		return nil, fmt.Errorf("LagProfile: lagLo <= lagHi")
	}
	if es := shardEngines(); es != nil {
		return nil, fmt.Errorf("LagProfile runs on one device")
	}
	e, err := getEngine()
	if err != nil {
		return nil, err
	}
	dg, err := b.Comparison.residentRows(e)
	if err != nil {
		return nil, err
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if b.batch == nil || b.batchGroup != dg {
		if b.batch != nil {
			C.muse_batch_free(b.batch)
		}
		st := C.muse_batch_create_like(b.template, dg, &b.batch)
		if err := hipError(st); err != nil {
			return nil, err
		}
		b.batchGroup = dg
	}
	W := lagHi - lagLo + 1
	K := len(b.Comparison.order)
	var list *C.int64_t
	var idx []C.int64_t
	if rows != nil {
		K = len(rows)
		idx = make([]C.int64_t, K+1) // (a list of no entries is still a list: a non-nil pointer)
		for i, r := range rows {
			idx[i] = C.int64_t(r)
		}
		list = &idx[0]
	}
	flat := make([]C.double, K*W+1)
	listed := C.int64_t(0)
	if rows != nil {
		listed = C.int64_t(K)
	}
	st := C.muse_batch_lag_profile(b.batch, list, listed, C.int32_t(lagLo), C.int32_t(lagHi), &flat[0], C.int64_t(W))
	runtime.KeepAlive(idx)
	if err := hipError(st); err != nil {
		return nil, err
	}
	out := make([][]float64, K)
	for k := range out {
		out[k] = make([]float64, W)
		for v := range out[k] {
			out[k][v] = float64(flat[k*W+v])
		}
	}
	return out, nil
}

// RunSigned is RunSignedInLagRange(-MaxLag, MaxLag): RunInWindow with Results.SignFilter restricting the argmax.
func (b *Batch) RunSigned(groupByLabels []string) error {
	if b.Results.MaxLag < 0 {
		return fmt.Errorf("RunSigned: MaxLag < 0")
	}
	return b.RunSignedInLagRange(groupByLabels, -b.Results.MaxLag, b.Results.MaxLag)
}

// feedInWindow is what RunInWindow, RunInLagRange and RunSignedInLagRange share: the label groups, the resident rows, the call (ranged:
// the lag range lagLo .. lagHi, otherwise the window Results.MaxLag; signed: the ranged call whose argmax takes Results.SignFilter) and
// the feed of Results in group order.  band: the lag band lagLo .. lagHi, which need not hold lag 0 (muse_batch_run_in_lag_band; signed as
// above, unsigned: the device always gets SignFilter_ANY, because the call's sign is the argmax's too).
func (b *Batch) feedInWindow(groupByLabels []string, ranged bool, lagLo, lagHi int, signed bool, band bool) error {
	labelValuesSet := b.Comparison.indexLabelValues(groupByLabels)
	if len(labelValuesSet) == 0 {
		return nil
	}
	pos := make(map[string]int, len(b.Comparison.order))
	for i, s := range b.Comparison.order {
		pos[s.UID()] = i
	}
	gid := make([]C.int32_t, len(b.Comparison.order))
	gi := 0
	for _, lv := range labelValuesSet {
		for _, uid := range b.Comparison.index[lv.ID(lv.Keys())] {
			gid[pos[uid]] = C.int32_t(gi)
		}
		gi++
	}
	e, err := getEngine()
	if err != nil {
		return err
	}
	dg, err := b.Comparison.residentRows(e)
	if err != nil {
		return err
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if b.batch == nil || b.batchGroup != dg {
		if b.batch != nil {
			C.muse_batch_free(b.batch)
		}
		st := C.muse_batch_create_like(b.template, dg, &b.batch)
		if err := hipError(st); err != nil {
			return err
		}
		b.batchGroup = dg
	}
	// (as Run does: a window an earlier RunWindowed left on the handle goes; this pass takes its own as an argument)
	if err := hipError(C.muse_batch_set_lag_window(b.batch, C.int32_t(b.window))); err != nil {
		return err
	}
	r := b.Results
	G := len(labelValuesSet)
	topN, threshold, sign := r.TopN, r.Threshold, int(r.SignFilter)
	if G <= exactFeedMaxGroups {
		topN, threshold, sign = G, 0.0, 0
	}
	top := topN
	if top < 1 {
		top = 1
	}
	idx := make([]C.int64_t, top)
	lag := make([]C.int32_t, top)
	score := make([]C.double, top)
	var cnt C.int32_t
	var mean C.double
	var st C.int
	if band {
		bandSign, absScores := 0, 1
		if signed && int(r.SignFilter) != 0 { // (not SignFilter_ANY)
			bandSign, absScores = int(r.SignFilter), 0
		}
		st = C.muse_batch_run_in_lag_band(b.batch, &gid[0], C.int32_t(G), C.int32_t(lagLo), C.int32_t(lagHi), C.int32_t(topN),
			C.double(threshold), C.int32_t(bandSign), C.int32_t(absScores), &idx[0], &lag[0], &score[0], &cnt, &mean)
	} else if signed {
		absScores := 1
		if int(r.SignFilter) != 0 { // (not SignFilter_ANY)
			absScores = 0
		}
		st = C.muse_batch_run_signed_in_lag_range(b.batch, &gid[0], C.int32_t(G), C.int32_t(lagLo), C.int32_t(lagHi), C.int32_t(topN),
			C.double(threshold), C.int32_t(r.SignFilter), C.int32_t(absScores), &idx[0], &lag[0], &score[0], &cnt, &mean)
	} else if ranged {
		st = C.muse_batch_run_in_lag_range(b.batch, &gid[0], C.int32_t(G), C.int32_t(lagLo), C.int32_t(lagHi), C.int32_t(topN),
			C.double(threshold), C.int32_t(sign), 1, &idx[0], &lag[0], &score[0], &cnt, &mean)
	} else {
		st = C.muse_batch_run_in_window(b.batch, &gid[0], C.int32_t(G), C.int32_t(r.MaxLag), C.int32_t(topN),
			C.double(threshold), C.int32_t(sign), 1, &idx[0], &lag[0], &score[0], &cnt, &mean)
	}
	if err := hipError(st); err != nil {
		return err
	}
	order := make([]int, int(cnt))
	for i := range order {
		order[i] = i
	}
	sort.SliceStable(order, func(a, c int) bool { return gid[idx[order[a]]] < gid[idx[order[c]]] })
	for _, k := range order {
		b.Results.Update(Score{Labels: b.Comparison.order[idx[k]].Labels(), Lag: int(lag[k]), PercentScore: float64(score[k])})
	}
	return nil
}

const exactFeedMaxGroups = 65536

// feedGroupWinners merges the shards' per-group records (muse_merge_group_winners: the first shard with a member decides the NaN
// rule, the maximum by |score| wins, the earlier shard on ties) and pushes one Score per label group through Results.Update in
// group order.  recs / state: nShards x G entries in C memory, shard-major.  Call with the OS thread locked.
func (b *Batch) feedGroupWinners(recs *C.muse_record, state *C.uint8_t, nShards, G int) error {
	win := (*C.muse_record)(C.calloc(C.size_t(G), C.size_t(unsafe.Sizeof(C.muse_record{}))))
	defer C.free(unsafe.Pointer(win))
	wst := (*C.uint8_t)(C.calloc(C.size_t(G), 1))
	defer C.free(unsafe.Pointer(wst))
	if err := hipError(C.muse_merge_group_winners(recs, state, C.int32_t(nShards), C.int32_t(G), win, wst)); err != nil {
		return err
	}
	winv := recView(win, G)
	wstv := u8View(wst, G)
	for g := 0; g < G; g++ {
		if wstv[g] != 1 { // 0: no member; 2: the group's score is NaN, which never passes Results.passed
			continue
		}
		w := winv[g]
		b.Results.Update(Score{Labels: b.Comparison.order[int(w.series)].Labels(), Lag: int(w.lag), PercentScore: float64(w.score)})
	}
	return nil
}

// runSharded is Run over several GPUs (SetDevices).  The Comparison group is cut into one contiguous row range per device
// and every shard is scored at the same time, one goroutine per device.  Label groups that live on ONE shard each
// (always true when every series is its own group): each shard returns its top-N candidates (muse_batch_run_shard,
// 24 B x TopN per device) and muse_merge_records selects.  Label groups that straddle shards: each shard returns its
// winner per group, unfiltered (muse_batch_run_groups), and muse_merge_group_records takes the per-group maximum BEFORE
// Results.passed and the top-N heap -- what SURVEY 8e requires for exactness.
func (b *Batch) runSharded(es []*engine, gid []C.int32_t, G int, exact bool) error {
	shards, err := b.Comparison.residentShards(es)
	if err != nil {
		return err
	}
	W := len(shards)
	if len(b.shardBatch) != W {
		for _, sb := range b.shardBatch {
			if sb != nil {
				C.muse_batch_free(sb)
			}
		}
		b.shardBatch = make([]*C.muse_batch, W)
		b.shardGroup = make([]*C.muse_group, W)
	}
	{
		runtime.LockOSThread()
		for r, sh := range shards {
			if b.shardBatch[r] == nil || b.shardGroup[r] != sh.g {
				if b.shardBatch[r] != nil {
					C.muse_batch_free(b.shardBatch[r])
					b.shardBatch[r] = nil
				}
				st := C.muse_batch_create(sh.e.ctx, sh.g, (*C.double)(unsafe.Pointer(&b.ref[0])), C.int32_t(len(b.ref)), &b.shardBatch[r])
				if err := hipError(st); err != nil {
					runtime.UnlockOSThread()
					return err
				}
				b.shardGroup[r] = sh.g
			}
			if err := hipError(C.muse_batch_set_lag_window(b.shardBatch[r], C.int32_t(b.window))); err != nil {
				runtime.UnlockOSThread()
				return err
			}
		}
		runtime.UnlockOSThread()
	}
	// does any label group have members on two shards?  (exact: every shard reports per group anyway)
	straddle := exact
	owner := make([]int, G)
	for i := range owner {
		owner[i] = -1
	}
	for r, sh := range shards {
		if exact {
			break
		}
		for i := sh.lo; i < sh.hi && !straddle; i++ {
			o := owner[gid[i]]
			if o >= 0 && o != r {
				straddle = true
			}
			owner[gid[i]] = r
		}
	}
	res := b.Results
	top := res.TopN
	capN := top
	if capN < 1 {
		capN = 1
	}
	per := capN
	if straddle {
		per = G
	}
	// C memory for what the devices write concurrently (muse_record is a plain 24-byte struct)
	recs := (*C.muse_record)(C.calloc(C.size_t(W*per), C.size_t(unsafe.Sizeof(C.muse_record{}))))
	defer C.free(unsafe.Pointer(recs))
	recv := recView(recs, W*per)
	var state *C.uint8_t
	var statev []C.uint8_t
	if straddle {
		state = (*C.uint8_t)(C.calloc(C.size_t(W*G), 1))
		defer C.free(unsafe.Pointer(state))
		statev = u8View(state, W*G)
	}
	cnt := make([]C.int32_t, W)
	errs := make([]error, W)
	var wg sync.WaitGroup
	for r, sh := range shards {
		if sh.lo == sh.hi {
			continue // an empty shard (fewer rows than devices)
		}
		wg.Add(1)
		go func(r int, sh *groupShard) {
			defer wg.Done()
			runtime.LockOSThread() // the cgo call and the muse_last_error that explains it: one OS thread
			defer runtime.UnlockOSThread()
			g := &gid[sh.lo]
			var st C.int
			if straddle {
				st = C.muse_batch_run_groups(b.shardBatch[r], g, C.int32_t(G), C.int64_t(sh.lo), 1, &recv[r*per],
					&statev[r*G])
			} else {
				st = C.muse_batch_run_shard(b.shardBatch[r], g, C.int32_t(G), C.int64_t(sh.lo), C.int32_t(res.MaxLag),
					C.int32_t(top), C.double(res.Threshold), C.int32_t(res.SignFilter), 1, &recv[r*per], &cnt[r])
			}
			errs[r] = hipError(st)
		}(r, sh)
	}
	wg.Wait()
	for _, e := range errs {
		if e != nil {
			return e
		}
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if exact {
		return b.feedGroupWinners(recs, state, W, G)
	}
	idx := make([]C.int64_t, capN)
	lag := make([]C.int32_t, capN)
	score := make([]C.double, capN)
	var n C.int32_t
	var mean C.double
	if straddle {
		st := C.muse_merge_group_records(recs, state, C.int32_t(W), C.int32_t(G), C.int32_t(res.MaxLag), C.int32_t(top),
			C.double(res.Threshold), C.int32_t(res.SignFilter), &idx[0], &lag[0], &score[0], &n, &mean)
		if err := hipError(st); err != nil {
			return err
		}
	} else {
		// compact the shards' candidate lists (count[r] of capN each) in place, then merge
		k := 0
		for r := 0; r < W; r++ {
			for i := 0; i < int(cnt[r]); i++ {
				recv[k] = recv[r*per+i]
				k++
			}
		}
		st := C.muse_merge_records(recs, C.int64_t(k), C.int32_t(top), &idx[0], &lag[0], &score[0], &n, &mean)
		if err := hipError(st); err != nil {
			return err
		}
	}
	order := make([]int, int(n))
	for i := range order {
		order[i] = i
	}
	sort.SliceStable(order, func(a, c int) bool { return gid[idx[order[a]]] < gid[idx[order[c]]] })
	for _, k := range order {
		b.Results.Update(Score{Labels: b.Comparison.order[idx[k]].Labels(), Lag: int(lag[k]), PercentScore: float64(score[k])})
	}
	return nil
}

// RunMany is Run for several batches that share one Comparison group and the
// same Results settings (README.md:10-13: many references against one set of
// series): the resident rows are read and forward-transformed once for all
// references (muse_batch_run_many).  Not part of the reference's API; batches
// that do not qualify are simply run one after the other.
func RunMany(batches []*Batch, groupByLabels []string) error {
	return runMany(batches, groupByLabels, false)
}

// RunManyWindowed is RunMany with the shared Results.MaxLag as a LAG WINDOW
// (muse_batch_run_many_windowed): every batch receives what its own
// RunWindowed gives, from one pass over the rows whose matrix product holds
// the windows of all references.  Batches that do not qualify for RunMany are
// RunWindowed one after the other.
func RunManyWindowed(batches []*Batch, groupByLabels []string) error {
	return runMany(batches, groupByLabels, true)
}

func runMany(batches []*Batch, groupByLabels []string, windowed bool) error {
	if len(batches) == 0 {
		return nil
	}
	b0 := batches[0]
	same := true
	for _, b := range batches {
		r, r0 := b.Results, b0.Results
		same = same && b.Comparison == b0.Comparison && r.MaxLag == r0.MaxLag && r.TopN == r0.TopN &&
			r.Threshold == r0.Threshold && r.SignFilter == r0.SignFilter
	}
	if !same {
		for _, b := range batches {
			run := b.Run
			if windowed {
				run = b.RunWindowed
			}
			if err := run(groupByLabels); err != nil {
				return err
			}
		}
		return nil
	}
	if windowed && (b0.Results.MaxLag < 0 || b0.Results.MaxLag > int(C.MUSE_LAG_WINDOW_MAX)) {
		return fmt.Errorf("RunManyWindowed: MaxLag outside 0 .. %d", int(C.MUSE_LAG_WINDOW_MAX))
	}
	labelValuesSet := b0.Comparison.indexLabelValues(groupByLabels)
	if len(labelValuesSet) == 0 {
		return nil
	}
	e, err := getEngine()
	if err != nil {
		return err
	}
	dg, err := b0.Comparison.residentRows(e)
	if err != nil {
		return err
	}
	pos := make(map[string]int, len(b0.Comparison.order))
	for i, s := range b0.Comparison.order {
		pos[s.UID()] = i
	}
	gid := make([]C.int32_t, len(b0.Comparison.order))
	gi := 0
	for _, lv := range labelValuesSet {
		for _, uid := range b0.Comparison.index[lv.ID(lv.Keys())] {
			gid[pos[uid]] = C.int32_t(gi)
		}
		gi++
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	// the handle array lives in C memory: cgo forbids passing Go memory that holds pointers
	R := len(batches)
	hs := (**C.muse_batch)(C.malloc(C.size_t(R) * C.size_t(unsafe.Sizeof((*C.muse_batch)(nil)))))
	defer C.free(unsafe.Pointer(hs))
	hv := batchView(hs, R)
	for i, b := range batches {
		if b.batch == nil || b.batchGroup != dg {
			if b.batch != nil {
				C.muse_batch_free(b.batch)
			}
			st := C.muse_batch_create(e.ctx, dg, (*C.double)(unsafe.Pointer(&b.ref[0])), C.int32_t(len(b.ref)), &b.batch)
			if err := hipError(st); err != nil {
				return err
			}
			b.batchGroup = dg
		}
		// (as Run does: a window an earlier RunWindowed left on the handle goes; the windowed pass takes its own as an argument)
		if err := hipError(C.muse_batch_set_lag_window(b.batch, C.int32_t(b.window))); err != nil {
			return err
		}
		hv[i] = b.batch
	}
	r := b0.Results
	top := r.TopN
	if top < 1 {
		top = 1
	}
	idx := make([]C.int64_t, R*top)
	lag := make([]C.int32_t, R*top)
	score := make([]C.double, R*top)
	cnt := make([]C.int32_t, R)
	mean := make([]C.double, R)
	var st C.int
	if windowed {
		st = C.muse_batch_run_many_windowed(hs, C.int32_t(R), &gid[0], C.int32_t(len(labelValuesSet)), C.int32_t(r.MaxLag),
			C.int32_t(r.TopN), C.double(r.Threshold), C.int32_t(r.SignFilter), 1, &idx[0], &lag[0], &score[0], &cnt[0], &mean[0])
	} else {
		st = C.muse_batch_run_many(hs, C.int32_t(R), &gid[0], C.int32_t(len(labelValuesSet)), C.int32_t(r.MaxLag),
			C.int32_t(r.TopN), C.double(r.Threshold), C.int32_t(r.SignFilter), 1, &idx[0], &lag[0], &score[0], &cnt[0], &mean[0])
	}
	if err := hipError(st); err != nil {
		return err
	}
	for i, b := range batches {
		o := i * r.TopN
		order := make([]int, int(cnt[i]))
		for k := range order {
			order[k] = k
		}
		sort.SliceStable(order, func(a, c int) bool { return gid[idx[o+order[a]]] < gid[idx[o+order[c]]] })
		for _, k := range order {
			b.Results.Update(Score{Labels: b.Comparison.order[idx[o+k]].Labels(), Lag: int(lag[o+k]), PercentScore: float64(score[o+k])})
		}
	}
	return nil
}

// RunManyInWindow is RunMany with the shared Results.MaxLag as a lag window of ANY width (muse_batch_run_many_in_window): every
// batch receives what its own RunInWindow gives, from one pass over the rows where the lengths have a masked many-references
// kernel (FFT lengths 512 ... 4096).  One device.  Results is fed as RunInWindow feeds it.  Batches that do not qualify for
// RunMany are RunInWindow one after the other.
func RunManyInWindow(batches []*Batch, groupByLabels []string) error {
	if len(batches) == 0 {
		return nil
	}
	maxLag := batches[0].Results.MaxLag
	return runManyInLags(batches, groupByLabels, "RunManyInWindow",
		func(b *Batch) error { return b.RunInWindow(groupByLabels) },
		func() error {
			if maxLag < 0 {
				return fmt.Errorf("RunManyInWindow: MaxLag < 0")
			}
			return nil
		},
		func(hs **C.muse_batch, R, G, topN C.int32_t, gid *C.int32_t, threshold C.double, sign C.int32_t, idx *C.int64_t,
			lag *C.int32_t, score *C.double, cnt *C.int32_t, mean *C.double) C.int {
			return C.muse_batch_run_many_in_window(hs, R, gid, G, C.int32_t(maxLag), topN, threshold, sign, 1, idx, lag, score, cnt, mean)
		})
}

// RunManyInLagRange is RunMany inside the lags lagLo .. lagHi, lagLo <= 0 <= lagHi (muse_batch_run_many_in_lag_range): every batch
// receives what its own RunInLagRange gives, from one pass over the rows -- up to 48 lags with the references' table rows packed
// into one matrix product.  One device.  Results is fed as RunInWindow feeds it.  Batches that do not qualify for RunMany are
// RunInLagRange one after the other.
func RunManyInLagRange(batches []*Batch, groupByLabels []string, lagLo, lagHi int) error {
	if lagLo > 0 || lagHi < 0 {
		return fmt.Errorf("RunManyInLagRange: lagLo <= 0 <= lagHi")
	}
	return runManyInLags(batches, groupByLabels, "RunManyInLagRange",
		func(b *Batch) error { return b.RunInLagRange(groupByLabels, lagLo, lagHi) },
		func() error { return nil },
		func(hs **C.muse_batch, R, G, topN C.int32_t, gid *C.int32_t, threshold C.double, sign C.int32_t, idx *C.int64_t,
			lag *C.int32_t, score *C.double, cnt *C.int32_t, mean *C.double) C.int {
			return C.muse_batch_run_many_in_lag_range(hs, R, gid, G, C.int32_t(lagLo), C.int32_t(lagHi), topN, threshold, sign, 1, idx,
				lag, score, cnt, mean)
		})
}

// RunManyInLagBand is RunMany inside the lag band lagLo .. lagHi, which need not hold lag 0 (muse_batch_run_many_in_lag_band): every
// batch receives what its own RunInLagBand gives -- the argmax by magnitude, the Results' own filters applied afterwards -- from
// one pass over the rows.  One device.  Batches that do not qualify for RunMany are RunInLagBand one after the other.
func RunManyInLagBand(batches []*Batch, groupByLabels []string, lagLo, lagHi int) error {
	if lagLo > lagHi {
		return fmt.Errorf("RunManyInLagBand: lagLo <= lagHi")
	}
	return runManyInLags(batches, groupByLabels, "RunManyInLagBand",
		func(b *Batch) error { return b.RunInLagBand(groupByLabels, lagLo, lagHi) },
		func() error { return nil },
		func(hs **C.muse_batch, R, G, topN C.int32_t, gid *C.int32_t, threshold C.double, sign C.int32_t, idx *C.int64_t,
			lag *C.int32_t, score *C.double, cnt *C.int32_t, mean *C.double) C.int {
			return C.muse_batch_run_many_in_lag_band(hs, R, gid, G, C.int32_t(lagLo), C.int32_t(lagHi), topN, threshold, 0, 1, idx,
				lag, score, cnt, mean)
		})
}

// RunManySignedInLagBand is RunManyInLagBand with the shared Results.SignFilter restricting the ARGMAX: every batch receives what
// its own RunSignedInLagBand gives; under a sign the Scores carry the signed value.  Batches that do not qualify are
// RunSignedInLagBand one after the other, each under its own filter.
func RunManySignedInLagBand(batches []*Batch, groupByLabels []string, lagLo, lagHi int) error {
	if lagLo > lagHi {
		return fmt.Errorf("RunManySignedInLagBand: lagLo <= lagHi")
	}
	if len(batches) == 0 {
		return nil
	}
	filter := C.int32_t(batches[0].Results.SignFilter)
	abs := C.int32_t(0)
	if filter == 0 {
		abs = 1
	}
	return runManyInLags(batches, groupByLabels, "RunManySignedInLagBand",
		func(b *Batch) error { return b.RunSignedInLagBand(groupByLabels, lagLo, lagHi) },
		func() error { return nil },
		func(hs **C.muse_batch, R, G, topN C.int32_t, gid *C.int32_t, threshold C.double, sign C.int32_t, idx *C.int64_t,
			lag *C.int32_t, score *C.double, cnt *C.int32_t, mean *C.double) C.int {
			return C.muse_batch_run_many_in_lag_band(hs, R, gid, G, C.int32_t(lagLo), C.int32_t(lagHi), topN, threshold, filter, abs,
				idx, lag, score, cnt, mean)
		})
}

// RunManyInLagBands is RunMany with a lag band PER BATCH (muse_batch_run_many_in_lag_bands): batch r receives what its own
// RunInLagBand(groupByLabels, bands[r][0], bands[r][1]) gives -- the argmax by magnitude, its own Results' filters applied
// afterwards -- from one pass over the rows.  The batches' Results may differ in every field.  One device.  Batches that do not
// share the Comparison are RunInLagBand one after the other.
func RunManyInLagBands(batches []*Batch, groupByLabels []string, bands [][2]int) error {
	return runManyInBands(batches, groupByLabels, bands, "RunManyInLagBands", false)
}

// RunManySignedInLagBands is RunManyInLagBands with each batch's OWN Results.SignFilter restricting its argmax: batch r receives
// what its own RunSignedInLagBand gives; under a sign the Scores carry the signed value.
func RunManySignedInLagBands(batches []*Batch, groupByLabels []string, bands [][2]int) error {
	return runManyInBands(batches, groupByLabels, bands, "RunManySignedInLagBands", true)
}

// RunManySigned is RunManySignedInLagBands with bands[r] = (-MaxLag_r, MaxLag_r): every batch receives what its own RunSigned
// gives, under its own Results.MaxLag, TopN, Threshold and SignFilter, from one pass over the rows.
func RunManySigned(batches []*Batch, groupByLabels []string) error {
	bands := make([][2]int, len(batches))
	for i, b := range batches {
		if b.Results.MaxLag < 0 {
			return fmt.Errorf("RunManySigned: MaxLag < 0")
		}
		bands[i] = [2]int{-b.Results.MaxLag, b.Results.MaxLag}
	}
	return runManyInBands(batches, groupByLabels, bands, "RunManySigned", true)
}

// runManyInBands is what the three share: the checks, the batches that share one Comparison (otherwise the single methods one
// after the other), and every Results fed in group order what its own single method feeds it -- up to exactFeedMaxGroups label
// groups every group's winner, beyond the device's pre-selection under the batch's OWN TopN and Threshold -- with the (sign,
// abs_scores) that method hands its device call.  The C call takes one abs_scores: under signs the batches that report magnitudes
// (SignFilterAny) and those that report signed values take one pass each.
func runManyInBands(batches []*Batch, groupByLabels []string, bands [][2]int, name string, signed bool) error {
	if len(batches) == 0 {
		return nil
	}
	if len(bands) != len(batches) {
		return fmt.Errorf("%s: one (lagLo, lagHi) per batch", name)
	}
	b0 := batches[0]
	same := true
	signs := make([]int, len(batches))
	for i, b := range batches {
		if bands[i][0] > bands[i][1] {
			return fmt.Errorf("%s: lagLo <= lagHi", name)
		}
		if signed {
			signs[i] = int(b.Results.SignFilter)
		}
		same = same && b.Comparison == b0.Comparison
	}
	if !same {
		for i, b := range batches {
			var err error
			if signed {
				err = b.RunSignedInLagBand(groupByLabels, bands[i][0], bands[i][1])
			} else {
				err = b.RunInLagBand(groupByLabels, bands[i][0], bands[i][1])
			}
			if err != nil {
				return err
			}
		}
		return nil
	}
	if es := shardEngines(); es != nil {
		return fmt.Errorf("%s runs on one device", name)
	}
	labelValuesSet := b0.Comparison.indexLabelValues(groupByLabels)
	if len(labelValuesSet) == 0 {
		return nil
	}
	e, err := getEngine()
	if err != nil {
		return err
	}
	dg, err := b0.Comparison.residentRows(e)
	if err != nil {
		return err
	}
	pos := make(map[string]int, len(b0.Comparison.order))
	for i, s := range b0.Comparison.order {
		pos[s.UID()] = i
	}
	gid := make([]C.int32_t, len(b0.Comparison.order))
	gi := 0
	for _, lv := range labelValuesSet {
		for _, uid := range b0.Comparison.index[lv.ID(lv.Keys())] {
			gid[pos[uid]] = C.int32_t(gi)
		}
		gi++
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	G := len(labelValuesSet)
	for pass := 0; pass < 2; pass++ { // the batches that report magnitudes, then those that report signed values
		var of []int
		for i := range batches {
			if (signs[i] == 0) == (pass == 0) {
				of = append(of, i)
			}
		}
		R := len(of)
		if R == 0 {
			continue
		}
		// the handle array lives in C memory: cgo forbids passing Go memory that holds pointers
		hs := (**C.muse_batch)(C.malloc(C.size_t(R) * C.size_t(unsafe.Sizeof((*C.muse_batch)(nil)))))
		defer C.free(unsafe.Pointer(hs))
		hv := batchView(hs, R)
		lo := make([]C.int32_t, R)
		hi := make([]C.int32_t, R)
		topN := make([]C.int32_t, R)
		sign := make([]C.int32_t, R)
		threshold := make([]C.double, R)
		stride := 1
		for k, i := range of {
			b := batches[i]
			if b.batch == nil || b.batchGroup != dg {
				if b.batch != nil {
					C.muse_batch_free(b.batch)
				}
				st := C.muse_batch_create(e.ctx, dg, (*C.double)(unsafe.Pointer(&b.ref[0])), C.int32_t(len(b.ref)), &b.batch)
				if err := hipError(st); err != nil {
					return err
				}
				b.batchGroup = dg
			}
			// (as Run does: a window an earlier RunWindowed left on the handle goes; this pass takes its own as an argument)
			if err := hipError(C.muse_batch_set_lag_window(b.batch, C.int32_t(b.window))); err != nil {
				return err
			}
			hv[k] = b.batch
			lo[k], hi[k], sign[k] = C.int32_t(bands[i][0]), C.int32_t(bands[i][1]), C.int32_t(signs[i])
			topN[k], threshold[k] = C.int32_t(b.Results.TopN), C.double(b.Results.Threshold)
			if G <= exactFeedMaxGroups {
				topN[k], threshold[k] = C.int32_t(G), 0.0
			}
			if int(topN[k]) > stride {
				stride = int(topN[k])
			}
		}
		abs := C.int32_t(0)
		if pass == 0 {
			abs = 1
		}
		idx := make([]C.int64_t, R*stride)
		lag := make([]C.int32_t, R*stride)
		score := make([]C.double, R*stride)
		cnt := make([]C.int32_t, R)
		mean := make([]C.double, R)
		st := C.muse_batch_run_many_in_lag_bands(hs, C.int32_t(R), &gid[0], C.int32_t(G), &lo[0], &hi[0], &topN[0], &threshold[0],
			&sign[0], abs, C.int32_t(stride), &idx[0], &lag[0], &score[0], &cnt[0], &mean[0])
		if err := hipError(st); err != nil {
			return err
		}
		for k, i := range of {
			b := batches[i]
			o := k * stride
			order := make([]int, int(cnt[k]))
			for j := range order {
				order[j] = j
			}
			sort.SliceStable(order, func(a, c int) bool { return gid[idx[o+order[a]]] < gid[idx[o+order[c]]] })
			for _, j := range order {
				b.Results.Update(Score{Labels: b.Comparison.order[idx[o+j]].Labels(), Lag: int(lag[o+j]), PercentScore: float64(score[o+j])})
			}
		}
	}
	return nil
}

// runManyInLags is what RunManyInWindow, RunManyInLagRange and RunManyInLagBand share: the batches that qualify (otherwise each, batch after batch),
// pre (the form's own refusal once they do), the label groups, the resident rows, the handles, the call (one of the library's
// _run_many_in_ entry points) and the feed of every Results in group order.
func runManyInLags(batches []*Batch, groupByLabels []string, name string, each func(*Batch) error, pre func() error,
	call func(hs **C.muse_batch, R, G, topN C.int32_t, gid *C.int32_t, threshold C.double, sign C.int32_t, idx *C.int64_t,
		lag *C.int32_t, score *C.double, cnt *C.int32_t, mean *C.double) C.int) error {
	if len(batches) == 0 {
		return nil
	}
	b0 := batches[0]
	same := true
	for _, b := range batches {
		r, r0 := b.Results, b0.Results
		same = same && b.Comparison == b0.Comparison && r.MaxLag == r0.MaxLag && r.TopN == r0.TopN &&
			r.Threshold == r0.Threshold && r.SignFilter == r0.SignFilter
	}
	if !same {
		for _, b := range batches {
			if err := each(b); err != nil {
				return err
			}
		}
		return nil
	}
	if err := pre(); err != nil {
		return err
	}
	if es := shardEngines(); es != nil {
		return fmt.Errorf("%s runs on one device", name)
	}
	labelValuesSet := b0.Comparison.indexLabelValues(groupByLabels)
	if len(labelValuesSet) == 0 {
		return nil
	}
	e, err := getEngine()
	if err != nil {
		return err
	}
	dg, err := b0.Comparison.residentRows(e)
	if err != nil {
		return err
	}
	pos := make(map[string]int, len(b0.Comparison.order))
	for i, s := range b0.Comparison.order {
		pos[s.UID()] = i
	}
	gid := make([]C.int32_t, len(b0.Comparison.order))
	gi := 0
	for _, lv := range labelValuesSet {
		for _, uid := range b0.Comparison.index[lv.ID(lv.Keys())] {
			gid[pos[uid]] = C.int32_t(gi)
		}
		gi++
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	// the handle array lives in C memory: cgo forbids passing Go memory that holds pointers
	R := len(batches)
	hs := (**C.muse_batch)(C.malloc(C.size_t(R) * C.size_t(unsafe.Sizeof((*C.muse_batch)(nil)))))
	defer C.free(unsafe.Pointer(hs))
	hv := batchView(hs, R)
	for i, b := range batches {
		if b.batch == nil || b.batchGroup != dg {
			if b.batch != nil {
				C.muse_batch_free(b.batch)
			}
			st := C.muse_batch_create(e.ctx, dg, (*C.double)(unsafe.Pointer(&b.ref[0])), C.int32_t(len(b.ref)), &b.batch)
			if err := hipError(st); err != nil {
				return err
			}
			b.batchGroup = dg
		}
		// (as Run does: a window an earlier RunWindowed left on the handle goes; this pass takes its own as an argument)
		if err := hipError(C.muse_batch_set_lag_window(b.batch, C.int32_t(b.window))); err != nil {
			return err
		}
		hv[i] = b.batch
	}
	r := b0.Results
	G := len(labelValuesSet)
	topN, threshold, sign := r.TopN, r.Threshold, int(r.SignFilter)
	if G <= exactFeedMaxGroups {
		topN, threshold, sign = G, 0.0, 0
	}
	top := topN
	if top < 1 {
		top = 1
	}
	idx := make([]C.int64_t, R*top)
	lag := make([]C.int32_t, R*top)
	score := make([]C.double, R*top)
	cnt := make([]C.int32_t, R)
	mean := make([]C.double, R)
	st := call(hs, C.int32_t(R), C.int32_t(G), C.int32_t(topN), &gid[0], C.double(threshold), C.int32_t(sign), &idx[0], &lag[0],
		&score[0], &cnt[0], &mean[0])
	if err := hipError(st); err != nil {
		return err
	}
	if topN < 0 {
		topN = 0
	}
	for i, b := range batches {
		o := i * topN
		order := make([]int, int(cnt[i]))
		for k := range order {
			order[k] = k
		}
		sort.SliceStable(order, func(a, c int) bool { return gid[idx[o+order[a]]] < gid[idx[o+order[c]]] })
		for _, k := range order {
			b.Results.Update(Score{Labels: b.Comparison.order[idx[o+k]].Labels(), Lag: int(lag[o+k]), PercentScore: float64(score[o+k])})
		}
	}
	return nil
}

// xCorrBatch is xCorr (xcorr.go:102-153) for many independent (x, y) pairs in ONE launch (muse_xcorr_batch; SURVEY 8f-4):
// xs[i] and ys[i] are pair i, every x of one length and every y of one length (each zero-padded on its own, xcorr.go:129-130),
// n raised to max(n, lenx, leny) as in xcorr.go:104-106.  Returns per pair the lag, the signed value and whether the
// reference would have returned (nil, 0, 0).  Unexported like xCorr itself: the package's tests are its callers
// (xcorr_test.go:86-202).  The rows are packed into C memory (no Go pointer crosses); inputs are not mutated (the reference's
// zNormalize mutates x and y in place).
func xCorrBatch(xs, ys [][]float64, n int, normalize bool) (lags []int, mvs []float64, isNil []bool, err error) {
	m := len(xs)
	if m == 0 || len(ys) != m {
		return nil, nil, nil, errors.New("xCorrBatch: xs and ys must hold the same, non-zero number of series")
	}
	lenx, leny := len(xs[0]), len(ys[0])
	for i := 0; i < m; i++ {
		if len(xs[i]) != lenx || len(ys[i]) != leny {
			return nil, nil, nil, errors.New("xCorrBatch: every x (and every y) must have one length")
		}
	}
	e, err := getEngine()
	if err != nil {
		return nil, nil, nil, err
	}
	bx := (*C.double)(C.malloc(C.size_t(m) * C.size_t(lenx) * 8))
	by := (*C.double)(C.malloc(C.size_t(m) * C.size_t(leny) * 8))
	clag := (*C.int32_t)(C.malloc(C.size_t(m) * 4))
	cnil := (*C.int32_t)(C.malloc(C.size_t(m) * 4))
	cmv := (*C.double)(C.malloc(C.size_t(m) * 8))
	defer C.free(unsafe.Pointer(bx))
	defer C.free(unsafe.Pointer(by))
	defer C.free(unsafe.Pointer(clag))
	defer C.free(unsafe.Pointer(cnil))
	defer C.free(unsafe.Pointer(cmv))
	if bx == nil || by == nil || clag == nil || cnil == nil || cmv == nil {
		return nil, nil, nil, errors.New("out of memory staging series for xCorrBatch")
	}
	sx := f64View(unsafe.Pointer(bx), m*lenx)
	sy := f64View(unsafe.Pointer(by), m*leny)
	for i := 0; i < m; i++ {
		copy(sx[i*lenx:(i+1)*lenx], xs[i])
		copy(sy[i*leny:(i+1)*leny], ys[i])
	}
	norm := C.int32_t(0)
	if normalize {
		norm = 1
	}
	if err := hipError(C.muse_xcorr_batch(e.ctx, bx, by, C.int64_t(m), C.int32_t(lenx), C.int32_t(leny), C.int32_t(n), norm,
		clag, cmv, cnil, nil)); err != nil {
		return nil, nil, nil, err
	}
	lags, mvs, isNil = make([]int, m), make([]float64, m), make([]bool, m)
	gl := i32View(unsafe.Pointer(clag), m)
	gn := i32View(unsafe.Pointer(cnil), m)
	gv := f64View(unsafe.Pointer(cmv), m)
	for i := 0; i < m; i++ {
		lags[i], mvs[i], isNil[i] = int(gl[i]), gv[i], gn[i] != 0
	}
	return lags, mvs, isNil, nil
}

// Muse keeps the exported fields of muse.go:13-17; x and n are gone (the
// reference spectrum lives on the device, owned by the template batch).
type Muse struct {
	Results  *Results
	ref      []float64
	probe    *C.muse_group // empty group the template batch is bound to
	template *C.muse_batch // owns the reference spectrum, shared by every Run
}

// New replaces muse.go:23-42: empty reference -> error, sigma(ref) == 0 ->
// "Invalid input query" error; the spectrum is computed once, here.
func New(ref *Series, results *Results) (*Muse, error) {
	if ref.Length() < 1 {
		return nil, errors.New("Reference series length must be greater than zero")
	}
	e, err := getEngine()
	if err != nil {
		return nil, err
	}
	m := &Muse{Results: results, ref: append([]float64(nil), ref.Values()...)}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if err := hipError(C.muse_group_create(e.ctx, 0, C.int32_t(len(m.ref)), &m.probe)); err != nil {
		return nil, err
	}
	st := C.muse_batch_create(e.ctx, m.probe, (*C.double)(unsafe.Pointer(&m.ref[0])), C.int32_t(len(m.ref)), &m.template)
	if err := hipError(st); err != nil {
		C.muse_group_free(m.probe)
		return nil, fmt.Errorf("Invalid input query, %v", err)
	}
	runtime.SetFinalizer(m, func(m *Muse) {
		C.muse_batch_free(m.template)
		C.muse_group_free(m.probe)
	})
	return m, nil
}

// Run replaces muse.go:46-92: one label group per call, signed score clamped
// to [-1, 1], the group's best |score| goes to Results.  Safe to call from many
// goroutines (muse_test.go:203-214): every call owns its group and batch, the
// spectrum is shared read-only, Results has its mutex.
func (m *Muse) Run(compGraphs []*Series) error {
	return m.run(compGraphs, -1, nil)
}

// RunWindowed is Run with Results.MaxLag as a LAG WINDOW (muse_batch_run_rows_windowed): every series contributes its best
// match inside +-MaxLag, where Run takes its best match over all lags and Update drops the group when that lies outside.
// The window is an argument of the call: Run itself never changes, and both may be in flight from many goroutines.
func (m *Muse) RunWindowed(compGraphs []*Series) error {
	if m.Results.MaxLag < 0 || m.Results.MaxLag > C.MUSE_LAG_WINDOW_MAX {
		return fmt.Errorf("RunWindowed: MaxLag outside 0 .. %d", int(C.MUSE_LAG_WINDOW_MAX))
	}
	return m.run(compGraphs, m.Results.MaxLag, nil)
}

// RunInLagRange is Run inside the lags lagLo .. lagHi, lagLo <= 0 <= lagHi (muse_batch_run_rows_in_lag_range): every series
// contributes its best match inside the range -- up to MUSE_RUN_ROWS_LAG_RANGE_MAX lags, one-sided ranges too ("which of these
// series trails the reference by up to k samples?").  Results is fed as Batch.RunInLagRange feeds it: the group's Score through
// Results.Update, which applies the Results' own filters unchanged.  The range is an argument of the call: Run itself never changes.
func (m *Muse) RunInLagRange(compGraphs []*Series, lagLo, lagHi int) error {
	if lagLo > 0 || lagHi < 0 {
		return fmt.Errorf("RunInLagRange: lagLo <= 0 <= lagHi")
	}
	return m.run(compGraphs, -1, &[2]int{lagLo, lagHi})
}

// lagRange != nil: RunInLagRange with those lags; else window < 0: Run; otherwise RunWindowed with that window
func (m *Muse) run(compGraphs []*Series, window int, lagRange *[2]int) error {
	if len(compGraphs) == 0 {
		return nil
	}
	N := len(m.ref)
	rows := make([]float64, 0, len(compGraphs)*N)
	for _, s := range compGraphs {
		if s.Length() != N { // muse.go:68-70
			return fmt.Errorf("Encountered a comparison graph with differing length than the reference, %v", s.Labels())
		}
		rows = append(rows, s.Values()...)
	}
	if _, err := getEngine(); err != nil {
		return err
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	// one ABI call: upload, fused kernel, group maximum, record back; signed scores (muse.go:72-76).  The rows are
	// copied before the call returns (cgo rule); Results.Update applies passed() as the reference does.
	var win C.muse_record
	var state C.uint8_t
	var st C.int
	if lagRange != nil {
		st = C.muse_batch_run_rows_in_lag_range(m.template, (*C.double)(unsafe.Pointer(&rows[0])), C.int64_t(len(compGraphs)), C.int64_t(N), C.int32_t(lagRange[0]), C.int32_t(lagRange[1]), 0, &win, &state)
	} else if window >= 0 {
		st = C.muse_batch_run_rows_windowed(m.template, (*C.double)(unsafe.Pointer(&rows[0])), C.int64_t(len(compGraphs)), C.int64_t(N), C.int32_t(window), 0, &win, &state)
	} else {
		st = C.muse_batch_run_rows(m.template, (*C.double)(unsafe.Pointer(&rows[0])), C.int64_t(len(compGraphs)), C.int64_t(N), 0, &win, &state)
	}
	if err := hipError(st); err != nil {
		return err
	}
	if state == 1 && win.series >= 0 {
		m.Results.Update(Score{Labels: compGraphs[win.series].Labels(), Lag: int(win.lag), PercentScore: float64(win.score)})
	}
	return nil
}
