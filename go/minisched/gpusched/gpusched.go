// Package gpusched is the Go side of the MI355X scheduling core: it packs the informer snapshot of
// v1.Node and v1.Pod objects into the SoA columns libminisched_hip.so reads and calls its C-ABI
// (include/minisched_hip.h) through cgo.
//
// It replaces the selection part of Scheduler.scheduleOne (minisched/minisched.go:40-87: the node
// LIST, RunFilterPlugins, RunPreScorePlugins, RunScorePlugins and selectHost) for a batch of pods
// drained from activeQ. Permit, Bind, the queue and the event handlers stay in Go, unchanged.
//
// The framework.*Plugin values stay the source of truth: New maps their Name()s to device plugin
// ids and reports ErrUnsupported for a plugin list the device path does not implement, in which
// case the caller keeps the reference's per-pod Go loop (minisched.go:115-199).
//
// Not compiled in the repository that ships this file (its build image has no Go toolchain): copy
// the go/minisched tree into the reference's minisched/ and build it with the module's own go.mod
// (k8s.io/kubernetes v1.22.0). See go/README.md.
package gpusched

/*
#cgo CFLAGS: -I${SRCDIR}/../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../../mini-kube-scheduler_amd -lminisched_hip -Wl,-rpath,${SRCDIR}/../../../mini-kube-scheduler_amd
#include <stdlib.h>
#include "minisched_hip.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"sort"
	"sync"
	"unsafe"

	v1 "k8s.io/api/core/v1"
	"k8s.io/apimachinery/pkg/labels"
	"k8s.io/apimachinery/pkg/util/sets"
	corelisters "k8s.io/client-go/listers/core/v1"
	"k8s.io/client-go/tools/cache"
	"k8s.io/kubernetes/pkg/scheduler/framework"
)

// ErrUnsupported: the plugin list names a plugin with no device implementation. The caller keeps
// the reference's Go loop for it.
var ErrUnsupported = errors.New("gpusched: plugin list not implemented on the device")

// Device ids of the framework.Plugin names the device path implements (initialize.go:80-123).
var (
	filterIDs   = map[string]C.int32_t{"NodeUnschedulable": C.MSH_PLUGIN_NODE_UNSCHEDULABLE}
	preScoreIDs = map[string]C.int32_t{"NodeNumber": C.MSH_PLUGIN_NODE_NUMBER}
	scoreIDs    = map[string]C.int32_t{"NodeNumber": C.MSH_PLUGIN_NODE_NUMBER}
)

// Normalize is the NormalizeScore stage of one score plugin (msh_normalize). NodeNumber has no
// ScoreExtensions (nodenumber.go:98-100): NormalizeNone reproduces the reference.
type Normalize int32

const (
	NormalizeNone           Normalize = C.MSH_NORMALIZE_NONE
	NormalizeDefault        Normalize = C.MSH_NORMALIZE_DEFAULT         // helper.DefaultNormalizeScore(100, false)
	NormalizeDefaultReverse Normalize = C.MSH_NORMALIZE_DEFAULT_REVERSE // helper.DefaultNormalizeScore(100, true)
	NormalizeMinMax         Normalize = C.MSH_NORMALIZE_MINMAX
)

// ScoreConfig is one entry of the score list. The reference has no weights ("TODO: plugin weight",
// minisched.go:187): Weight 1 reproduces it.
type ScoreConfig struct {
	Plugin    framework.ScorePlugin
	Weight    int64
	Normalize Normalize
}

// Scores is the reference's score list as device entries: weight 1, no normalize (minisched.go:164-199).
func Scores(plugins []framework.ScorePlugin) []ScoreConfig {
	out := make([]ScoreConfig, len(plugins))
	for i, p := range plugins {
		out[i] = ScoreConfig{Plugin: p, Weight: 1, Normalize: NormalizeNone}
	}
	return out
}

// Ctx is one device context (one per GPU; not safe for concurrent use: give each goroutine that
// submits its own Ctx, locked to its OS thread or not — every entry point sets the device).
type Ctx struct {
	c        *C.msh_ctx
	byIndex  []*v1.Node // device node index -> node (List order)
	hasNodes bool
}

func (x *Ctx) lastErr(what string, rc C.int) error {
	return fmt.Errorf("%s: %d: %s", what, int(rc), C.GoString(C.msh_last_error(x.c)))
}

// New creates a device context for `device` and installs the plugin lists (Scheduler.filterPlugins,
// preScorePlugins, scorePlugins; initialize.go:25-27).
func New(device int, filters []framework.FilterPlugin, preScores []framework.PreScorePlugin, scores []ScoreConfig) (*Ctx, error) {
	fids := make([]C.int32_t, 0, len(filters))
	for _, p := range filters {
		id, ok := filterIDs[p.Name()]
		if !ok {
			return nil, fmt.Errorf("%w: filter %q", ErrUnsupported, p.Name())
		}
		fids = append(fids, id)
	}
	pids := make([]C.int32_t, 0, len(preScores))
	for _, p := range preScores {
		id, ok := preScoreIDs[p.Name()]
		if !ok {
			return nil, fmt.Errorf("%w: pre-score %q", ErrUnsupported, p.Name())
		}
		pids = append(pids, id)
	}
	sids := make([]C.int32_t, 0, len(scores))
	ws := make([]C.int64_t, 0, len(scores))
	norms := make([]C.int32_t, 0, len(scores))
	for _, s := range scores {
		id, ok := scoreIDs[s.Plugin.Name()]
		if !ok {
			return nil, fmt.Errorf("%w: score %q", ErrUnsupported, s.Plugin.Name())
		}
		w := s.Weight
		if w == 0 {
			w = 1
		}
		sids = append(sids, id)
		ws = append(ws, C.int64_t(w))
		norms = append(norms, C.int32_t(s.Normalize))
	}
	var c *C.msh_ctx
	if rc := C.msh_create(C.int(device), &c); rc != C.MSH_OK {
		return nil, fmt.Errorf("msh_create(%d): %d: %s", device, int(rc), C.GoString(C.msh_last_error(nil)))
	}
	x := &Ctx{c: c}
	if rc := C.msh_set_plugins_ex(c, ptrI32(fids), C.int32_t(len(fids)), ptrI32(pids), C.int32_t(len(pids)),
		ptrI32(sids), ptrI64(ws), ptrI32(norms), C.int32_t(len(sids))); rc != C.MSH_OK {
		err := x.lastErr("msh_set_plugins_ex", rc)
		C.msh_destroy(c)
		return nil, err
	}
	runtime.SetFinalizer(x, (*Ctx).Close)
	return x, nil
}

// Close releases the device context. Batches in flight are waited for.
func (x *Ctx) Close() {
	if x.c != nil {
		C.msh_destroy(x.c)
		x.c = nil
	}
	runtime.SetFinalizer(x, nil)
}

// TieBreak is selectHost's choice among the maximum-score nodes (msh_tiebreak).
type TieBreak int32

const (
	TieBreakFirst  TieBreak = C.MSH_TIEBREAK_FIRST  // the first maximum in List order (the default)
	TieBreakRandom TieBreak = C.MSH_TIEBREAK_RANDOM // uniform among the maxima, as the reference's reservoir scan
)

// SetTieBreak selects the tie-break of the batch calls (ScheduleBatch, Submit). TieBreakRandom places a
// pod on a uniformly drawn node of its tie set (minisched.go:304-325's distribution), the draw being
// SplitMix64(seed) at counter + the pod's position in the batch; each batch advances the counter by its
// pod count. ScheduleSequential, ScheduleNodeShard and Group.ScheduleBatch fail in that mode.
func (x *Ctx) SetTieBreak(mode TieBreak, seed, counter uint64) error {
	if rc := C.msh_set_tiebreak(x.c, C.int32_t(mode), C.uint64_t(seed), C.uint64_t(counter)); rc != C.MSH_OK {
		return x.lastErr("msh_set_tiebreak", rc)
	}
	return nil
}

// TieBreak returns the mode, the seed and the live draw counter (checkpoint it to replay a batch).
func (x *Ctx) TieBreak() (mode TieBreak, seed, counter uint64, err error) {
	var m C.int32_t
	var s, c C.uint64_t
	if rc := C.msh_get_tiebreak(x.c, &m, &s, &c); rc != C.MSH_OK {
		return TieBreakFirst, 0, 0, x.lastErr("msh_get_tiebreak", rc)
	}
	return TieBreak(m), uint64(s), uint64(c), nil
}

// UploadNodes replaces the per-cycle Nodes().List (minisched.go:40): the nodes are put in List
// order (byte-sorted names, the apiserver's etcd key order) and their two columns uploaded.
// It returns the device-index -> node mapping, also kept for ScheduleBatch.
func (x *Ctx) UploadNodes(nodes []v1.Node) ([]*v1.Node, error) {
	sorted := make([]*v1.Node, len(nodes))
	for i := range nodes {
		sorted[i] = &nodes[i]
	}
	sort.Slice(sorted, func(a, b int) bool { return sorted[a].Name < sorted[b].Name }) // Go string order == bytes
	uns := make([]C.uint8_t, len(sorted))
	dig := make([]C.int8_t, len(sorted))
	for i, n := range sorted {
		if n.Spec.Unschedulable {
			uns[i] = 1
		}
		dig[i] = C.int8_t(suffixDigit(n.Name))
	}
	if rc := C.msh_upload_nodes(x.c, C.int32_t(len(sorted)), ptrU8(uns), ptrI8(dig)); rc != C.MSH_OK {
		return nil, x.lastErr("msh_upload_nodes", rc)
	}
	x.byIndex, x.hasNodes = sorted, true
	return sorted, nil
}

// UpdateNode applies an informer Update that keeps the node's name (eventhandler.go:45-50, e.g. a
// cordon flipping Spec.Unschedulable) in O(1) host->device traffic. Adds, deletes and renames
// change List positions: call UploadNodes for those.
func (x *Ctx) UpdateNode(n *v1.Node) error { return x.UpdateNodes([]*v1.Node{n}) }

// UpdateNodes is UpdateNode for several nodes in one msh_patch_nodes call.
func (x *Ctx) UpdateNodes(nodes []*v1.Node) error {
	if len(nodes) == 0 {
		return nil
	}
	idx := make([]C.int32_t, len(nodes))
	uns := make([]C.uint8_t, len(nodes))
	dig := make([]C.int8_t, len(nodes))
	for k, n := range nodes {
		i := sort.Search(len(x.byIndex), func(q int) bool { return x.byIndex[q].Name >= n.Name })
		if i == len(x.byIndex) || x.byIndex[i].Name != n.Name {
			return fmt.Errorf("gpusched: node %q is not in the uploaded snapshot", n.Name)
		}
		idx[k] = C.int32_t(i)
		if n.Spec.Unschedulable {
			uns[k] = 1
		}
		dig[k] = C.int8_t(suffixDigit(n.Name))
	}
	if rc := C.msh_patch_nodes(x.c, C.int32_t(len(nodes)), ptrI32(idx), ptrU8(uns), ptrI8(dig)); rc != C.MSH_OK {
		return x.lastErr("msh_patch_nodes", rc)
	}
	// Copy on write: a HostBatch in flight keeps the mapping (and the node objects) of the table version
	// it was launched on; the names and List positions are the same, so either decodes the same index.
	byIndex := append([]*v1.Node(nil), x.byIndex...)
	for k, n := range nodes {
		byIndex[idx[k]] = n
	}
	x.byIndex = byIndex
	return nil
}

// NodeSnapshot keeps a Ctx's node table in step with the Node informer (eventhandler.go:45-65)
// instead of a LIST per cycle (minisched.go:40): an Add or a Delete changes List positions and marks
// the table for one full upload; an Update of an existing name (a cordon flip, or any other field
// change) queues an O(1) patch. Sync brings the Ctx up to date before a batch. The handlers run on
// the informer's goroutine, Sync on the scheduling loop's: both take the lock. Register it next to
// the reference's own handlers (which requeue pods on Node events):
//
//	snap := gpusched.NewNodeSnapshot()
//	informerFactory.Core().V1().Nodes().Informer().AddEventHandler(snap.Handlers())
//
// The Python mirror is mini-kube-scheduler_amd/nodecache.py (NodeCache.sync).
//
// A structural upload reads the informer's store through its lister when one is given
// (NewNodeSnapshotFromLister): WaitForCacheSync (scheduler.go:72-75) returns once the store holds the
// initial LIST, which can be before the handlers have been called for all of it, so a map filled by
// the handlers alone could upload a partial node list for the first batches, where the reference's
// per-cycle LIST (minisched.go:40) always sees every node. Handler calls that arrive after such an
// upload for nodes it already holds are then Updates: patches of identical values.
type NodeSnapshot struct {
	mu         sync.Mutex
	lister     corelisters.NodeLister // the informer's store (nil: the handlers' map alone)
	nodes      map[string]*v1.Node
	structural bool                // List positions changed since the last Sync
	patched    map[string]*v1.Node // names updated in place since the last Sync
}

// NewNodeSnapshot starts empty and structurally dirty: the first Sync uploads.
func NewNodeSnapshot() *NodeSnapshot {
	return &NodeSnapshot{nodes: map[string]*v1.Node{}, structural: true, patched: map[string]*v1.Node{}}
}

// NewNodeSnapshotFromLister is NewNodeSnapshot whose structural uploads read the informer's store:
//
//	nodes := informerFactory.Core().V1().Nodes()
//	snap := gpusched.NewNodeSnapshotFromLister(nodes.Lister())
//	nodes.Informer().AddEventHandler(snap.Handlers())
func NewNodeSnapshotFromLister(l corelisters.NodeLister) *NodeSnapshot {
	s := NewNodeSnapshot()
	s.lister = l
	return s
}

// Handlers are the informer callbacks (a cache.ResourceEventHandler).
func (s *NodeSnapshot) Handlers() cache.ResourceEventHandlerFuncs {
	return cache.ResourceEventHandlerFuncs{AddFunc: s.OnAdd, UpdateFunc: s.OnUpdate, DeleteFunc: s.OnDelete}
}

// OnAdd: a new name is a structural change; an Add for a name already present is an Update.
func (s *NodeSnapshot) OnAdd(obj interface{}) {
	n, ok := obj.(*v1.Node)
	if !ok {
		return
	}
	s.mu.Lock()
	defer s.mu.Unlock()
	if _, had := s.nodes[n.Name]; had {
		s.nodes[n.Name] = n
		s.patched[n.Name] = n
		return
	}
	s.nodes[n.Name] = n
	s.structural = true
}

// OnUpdate: names are immutable, so an Update keeps the node's List position: a patch.
func (s *NodeSnapshot) OnUpdate(_, newObj interface{}) {
	n, ok := newObj.(*v1.Node)
	if !ok {
		return
	}
	s.mu.Lock()
	defer s.mu.Unlock()
	if _, had := s.nodes[n.Name]; !had {
		s.nodes[n.Name] = n
		s.structural = true
		return
	}
	s.nodes[n.Name] = n
	s.patched[n.Name] = n
}

// OnDelete: every later List position shifts: a structural change.
func (s *NodeSnapshot) OnDelete(obj interface{}) {
	var name string
	switch t := obj.(type) {
	case *v1.Node:
		name = t.Name
	case cache.DeletedFinalStateUnknown:
		n, ok := t.Obj.(*v1.Node)
		if !ok {
			return
		}
		name = n.Name
	default:
		return
	}
	s.mu.Lock()
	defer s.mu.Unlock()
	if _, had := s.nodes[name]; had {
		delete(s.nodes, name)
		delete(s.patched, name)
		s.structural = true
	}
}

// Sync brings x's device table up to date: "upload" (msh_upload_nodes of every node, after an Add
// or a Delete), "patch" (msh_patch_nodes of the updated nodes only) or "clean".
func (s *NodeSnapshot) Sync(x *Ctx) (string, error) {
	s.mu.Lock()
	defer s.mu.Unlock()
	if s.structural {
		if s.lister != nil { // the store, consistent with HasSynced, replaces what the handlers have seen
			listed, err := s.lister.List(labels.Everything())
			if err != nil {
				return "", err
			}
			s.nodes = make(map[string]*v1.Node, len(listed))
			for _, n := range listed {
				s.nodes[n.Name] = n
			}
		}
		all := make([]v1.Node, 0, len(s.nodes))
		for _, n := range s.nodes {
			all = append(all, *n)
		}
		if _, err := x.UploadNodes(all); err != nil {
			return "", err
		}
		s.structural = false
		s.patched = map[string]*v1.Node{}
		return "upload", nil
	}
	if len(s.patched) > 0 {
		upd := make([]*v1.Node, 0, len(s.patched))
		for _, n := range s.patched {
			upd = append(upd, n)
		}
		if err := x.UpdateNodes(upd); err != nil {
			return "", err
		}
		s.patched = map[string]*v1.Node{}
		return "patch", nil
	}
	return "clean", nil
}

// Result of scheduleOne's selection part (minisched.go:50-87) for one pod.
type Result struct {
	Node   *v1.Node            // set when placed (selectHost's choice: the first maximum in List order)
	Score  int64               // the selected node's total score
	FitErr *framework.FitError // RunFilterPlugins found no feasible node (minisched.go:143-148)
	Err    error               // a Score plugin failed (minisched.go:70-75); ErrorFunc gets the nil filter error
}

// HostBatch holds one batch's pod columns and outputs in page-locked C memory (msh_host_alloc), so
// msh_schedule_batch copies nothing on the host: the kernel reads the columns and writes the outputs
// over PCIe. It is C memory, so the cgo pointer rules do not apply to it. Allocate once, reuse.
type HostBatch struct {
	cap         int
	mem         unsafe.Pointer
	pd          []C.int8_t
	pt          []C.uint8_t
	idx, status []C.int32_t
	score       []C.int64_t
	ticket      C.uint64_t // the pending msh_schedule_batch_async ticket, 0 = none
	pods        []*v1.Pod
	byIndex     []*v1.Node // the Ctx's device index -> node mapping when the batch was launched
}

// NewHostBatch allocates a HostBatch for up to `cap` pods (18 B per pod).
func NewHostBatch(cap int) (*HostBatch, error) {
	var mem unsafe.Pointer
	// score | idx | status | digit | tol: 8-byte aligned sections
	if rc := C.msh_host_alloc(C.size_t(18*cap+16), &mem); rc != C.MSH_OK {
		return nil, fmt.Errorf("msh_host_alloc(%d pods): %d", cap, int(rc))
	}
	b := &HostBatch{cap: cap, mem: mem}
	base := uintptr(mem)
	b.score = unsafe.Slice((*C.int64_t)(unsafe.Pointer(base)), cap)
	b.idx = unsafe.Slice((*C.int32_t)(unsafe.Pointer(base+uintptr(8*cap))), cap)
	b.status = unsafe.Slice((*C.int32_t)(unsafe.Pointer(base+uintptr(12*cap))), cap)
	b.pd = unsafe.Slice((*C.int8_t)(unsafe.Pointer(base+uintptr(16*cap))), cap)
	b.pt = unsafe.Slice((*C.uint8_t)(unsafe.Pointer(base+uintptr(17*cap))), cap)
	runtime.SetFinalizer(b, func(b *HostBatch) { C.msh_host_free(b.mem) })
	return b, nil
}

// pack writes the pods' PreScore / Filter inputs: the name suffix digit (NodeNumber.PreScore,
// nodenumber.go:50-64) and whether the tolerations tolerate the unschedulable taint
// (NodeUnschedulable.Filter, upstream v1.22.0), and keeps the Ctx's current index -> node mapping:
// the launch reads the table version published now, so its indices decode against this mapping even
// if UploadNodes replaces it before Wait (an upload builds a new slice; UpdateNodes keeps names and
// positions).
func (x *Ctx) pack(b *HostBatch, pods []*v1.Pod) error {
	if len(pods) > b.cap {
		return fmt.Errorf("gpusched: batch of %d pods exceeds the HostBatch capacity %d", len(pods), b.cap)
	}
	for j, pod := range pods {
		b.pd[j] = C.int8_t(suffixDigit(pod.Name))
		b.pt[j] = 0
		if tolerates(pod.Spec.Tolerations) {
			b.pt[j] = 1
		}
	}
	b.pods = pods
	b.byIndex = x.byIndex
	return nil
}

// results decodes the outputs with the reference's error routing (minisched.go:50-75,
// ErrorFunc :283-298).
func (x *Ctx) results(b *HostBatch) []Result {
	out := make([]Result, len(b.pods))
	for j, pod := range b.pods {
		switch b.status[j] {
		case C.MSH_PLACED:
			out[j] = Result{Node: b.byIndex[b.idx[j]], Score: int64(b.score[j])}
		case C.MSH_FIT_ERROR:
			diag := framework.Diagnosis{NodeToStatusMap: framework.NodeToStatusMap{}, UnschedulablePlugins: sets.NewString()}
			if len(b.byIndex) > 0 { // some node failed NodeUnschedulable
				diag.UnschedulablePlugins.Insert("NodeUnschedulable")
			}
			out[j] = Result{FitErr: &framework.FitError{Pod: pod, Diagnosis: diag}} // as minisched.go:143-148
		default:
			out[j] = Result{Err: framework.AsStatus(framework.ErrNotFound).AsError()}
		}
	}
	return out
}

// ScheduleBatch runs minisched.go:50-87 for every pod against the uploaded snapshot, synchronously.
func (x *Ctx) ScheduleBatch(pods []*v1.Pod, b *HostBatch) ([]Result, error) {
	if !x.hasNodes {
		return nil, errors.New("gpusched: UploadNodes has not been called")
	}
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	p := len(pods)
	if rc := C.msh_schedule_batch(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), ptrI32(b.idx[:p]),
		ptrI64(b.score[:p]), ptrI32(b.status[:p])); rc != C.MSH_OK {
		return nil, x.lastErr("msh_schedule_batch", rc)
	}
	return x.results(b), nil
}

// Submit launches a batch asynchronously (msh_schedule_batch_async) and returns at once: the caller
// packs and submits the next drained batch into another HostBatch while this one runs. Collect it
// with Wait. Batches of one Ctx complete in submission order.
func (x *Ctx) Submit(pods []*v1.Pod, b *HostBatch) error {
	if !x.hasNodes {
		return errors.New("gpusched: UploadNodes has not been called")
	}
	if b.ticket != 0 {
		return errors.New("gpusched: HostBatch has a batch in flight; Wait for it first")
	}
	if err := x.pack(b, pods); err != nil {
		return err
	}
	p := len(pods)
	if rc := C.msh_schedule_batch_async(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), ptrI32(b.idx[:p]),
		ptrI64(b.score[:p]), ptrI32(b.status[:p]), &b.ticket); rc != C.MSH_OK {
		b.ticket = 0
		return x.lastErr("msh_schedule_batch_async", rc)
	}
	return nil
}

// Wait returns the results of the batch last submitted into b.
func (x *Ctx) Wait(b *HostBatch) ([]Result, error) {
	if b.ticket == 0 {
		return nil, errors.New("gpusched: no batch in flight in this HostBatch")
	}
	t := b.ticket
	b.ticket = 0
	if rc := C.msh_wait(x.c, t); rc != C.MSH_OK {
		return nil, x.lastErr("msh_wait", rc)
	}
	return x.results(b), nil
}

// ScheduleSequential places the pods one at a time with a node-state commit between placements
// (the reference's serial Run loop, minisched.go:28-30, on the device). maxPodsPerNode > 0 makes a
// node infeasible once it holds that many pods (build extension); 0 = reference semantics, where no
// commit feeds a later decision: the library then runs the batch kernel and adds the placements to the
// node counts (a no-capacity shortcut with the serial loop's placements and counts).
func (x *Ctx) ScheduleSequential(pods []*v1.Pod, b *HostBatch, maxPodsPerNode int32) ([]Result, error) {
	if !x.hasNodes {
		return nil, errors.New("gpusched: UploadNodes has not been called")
	}
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	p := len(pods)
	if rc := C.msh_schedule_sequential(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), C.int32_t(maxPodsPerNode),
		ptrI32(b.idx[:p]), ptrI64(b.score[:p]), ptrI32(b.status[:p]), nil, nil); rc != C.MSH_OK {
		return nil, x.lastErr("msh_schedule_sequential", rc)
	}
	return x.results(b), nil
}

// ---- per-node pod capacity for ScheduleSequential (status.allocatable.pods) ----
//
// caps holds one value per uploaded node in List order (the order UploadNodes returned), 0 <= cap <=
// math.MaxInt32 (in effect unlimited). With a column ScheduleSequential stops at min(cap[i], maxPodsPerNode)
// per node, or at cap[i] alone when maxPodsPerNode is 0. UploadNodes drops the column; UpdateNodes keeps it;
// ScheduleBatch ignores it. Like the rest of this package these calls have not been compiled (go/README.md).

// UploadNodeCapacity sets the capacity column.
func (x *Ctx) UploadNodeCapacity(caps []int32) error {
	c := make([]C.int32_t, len(caps))
	for i, v := range caps {
		c[i] = C.int32_t(v)
	}
	if rc := C.msh_upload_node_capacity(x.c, C.int32_t(len(c)), ptrI32(c)); rc != C.MSH_OK {
		return x.lastErr("msh_upload_node_capacity", rc)
	}
	return nil
}

// PatchNodeCapacity replaces the capacities of the nodes at idx (distinct List-order indices); nothing is rebuilt.
func (x *Ctx) PatchNodeCapacity(idx, caps []int32) error {
	if len(idx) != len(caps) {
		return errors.New("gpusched: idx / caps length mismatch")
	}
	ci, cc := make([]C.int32_t, len(idx)), make([]C.int32_t, len(caps))
	for k := range idx {
		ci[k], cc[k] = C.int32_t(idx[k]), C.int32_t(caps[k])
	}
	if rc := C.msh_patch_node_capacity(x.c, C.int32_t(len(ci)), ptrI32(ci), ptrI32(cc)); rc != C.MSH_OK {
		return x.lastErr("msh_patch_node_capacity", rc)
	}
	return nil
}

// ClearNodeCapacity goes back to "no column".
func (x *Ctx) ClearNodeCapacity() error {
	if rc := C.msh_clear_node_capacity(x.c); rc != C.MSH_OK {
		return x.lastErr("msh_clear_node_capacity", rc)
	}
	return nil
}

// NodeCapacity returns the column (n entries, the uploaded node count), or nil when none is present.
func (x *Ctx) NodeCapacity(n int) ([]int32, error) {
	var present C.int32_t
	c := make([]C.int32_t, n)
	if rc := C.msh_node_capacity(x.c, ptrI32(c), &present); rc != C.MSH_OK {
		return nil, x.lastErr("msh_node_capacity", rc)
	}
	if present == 0 {
		return nil, nil
	}
	out := make([]int32, n)
	for i, v := range c {
		out[i] = int32(v)
	}
	return out, nil
}

// ---- resource requests for sequential mode (NodeResourcesFit: allocatable, used, requests) ----
//
// Amounts are int64 in [0, 2^62], resource-major (a[r*n+i]) in List order, in the caller's units (milli-cpu,
// bytes). ScheduleSequentialFit places a pod only where every amount it asks for fits alloc - used, and adds its
// requests to used. UploadNodes drops the table; UpdateNodes keeps it; every other call ignores it. Like the rest
// of this package these calls have not been compiled (go/README.md).

func toI64(v []int64) []C.int64_t {
	c := make([]C.int64_t, len(v))
	for i, x := range v {
		c[i] = C.int64_t(x)
	}
	return c
}

// UploadNodeResources sets the table: alloc (and used, nil = zeros) hold nres*n values.
func (x *Ctx) UploadNodeResources(n, nres int, alloc, used []int64) error {
	if len(alloc) != n*nres || (used != nil && len(used) != n*nres) {
		return errors.New("gpusched: alloc / used hold nres*n values")
	}
	if rc := C.msh_upload_node_resources(x.c, C.int32_t(n), C.int32_t(nres), ptrI64(toI64(alloc)), ptrI64(toI64(used))); rc != C.MSH_OK {
		return x.lastErr("msh_upload_node_resources", rc)
	}
	return nil
}

// PatchNodeResources replaces the values of the nodes at idx (distinct List-order indices): alloc / used hold
// nres*len(idx) values (a[r*len(idx)+k]), nil keeps that array. Nothing is rebuilt.
func (x *Ctx) PatchNodeResources(idx []int32, alloc, used []int64) error {
	ci := make([]C.int32_t, len(idx))
	for k := range idx {
		ci[k] = C.int32_t(idx[k])
	}
	if rc := C.msh_patch_node_resources(x.c, C.int32_t(len(ci)), ptrI32(ci), ptrI64(toI64(alloc)), ptrI64(toI64(used))); rc != C.MSH_OK {
		return x.lastErr("msh_patch_node_resources", rc)
	}
	return nil
}

// ClearNodeResources goes back to "no table".
func (x *Ctx) ClearNodeResources() error {
	if rc := C.msh_clear_node_resources(x.c); rc != C.MSH_OK {
		return x.lastErr("msh_clear_node_resources", rc)
	}
	return nil
}

// NodeResources returns nres, alloc and used (nres*n values each, n the uploaded node count), or nres = 0 when no
// table is present.
func (x *Ctx) NodeResources(n int) (nres int, alloc, used []int64, err error) {
	var present, nr C.int32_t
	a, u := make([]C.int64_t, n*int(C.MSH_MAX_RESOURCES)), make([]C.int64_t, n*int(C.MSH_MAX_RESOURCES))
	if rc := C.msh_node_resources(x.c, &nr, ptrI64(a), ptrI64(u), &present); rc != C.MSH_OK {
		return 0, nil, nil, x.lastErr("msh_node_resources", rc)
	}
	if present == 0 {
		return 0, nil, nil, nil
	}
	nres = int(nr)
	alloc, used = make([]int64, nres*n), make([]int64, nres*n)
	for i := range alloc {
		alloc[i], used[i] = int64(a[i]), int64(u[i])
	}
	return nres, alloc, used, nil
}

// ScheduleSequentialFit is ScheduleSequential with per-pod requests: req holds nres*len(pods) values
// (req[r*len(pods)+j]).
func (x *Ctx) ScheduleSequentialFit(pods []*v1.Pod, b *HostBatch, nres int, req []int64, maxPodsPerNode int32) ([]Result, error) {
	if !x.hasNodes {
		return nil, errors.New("gpusched: UploadNodes has not been called")
	}
	if len(req) != nres*len(pods) {
		return nil, errors.New("gpusched: req holds nres*len(pods) values")
	}
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	p := len(pods)
	if rc := C.msh_schedule_sequential_fit(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), C.int32_t(nres),
		ptrI64(toI64(req)), C.int32_t(maxPodsPerNode), ptrI32(b.idx[:p]), ptrI64(b.score[:p]), ptrI32(b.status[:p]), nil, nil); rc != C.MSH_OK {
		return nil, x.lastErr("msh_schedule_sequential_fit", rc)
	}
	return x.results(b), nil
}

// ScheduleSequentialFitDevice is the asynchronous form over device pointers (msh_schedule_sequential_fit_device);
// dReq is not validated by the library.
func (x *Ctx) ScheduleSequentialFitDevice(p int, dPodDigit, dPodTol unsafe.Pointer, nres int, dReq unsafe.Pointer,
	maxPodsPerNode int32, dIdx, dScore, dStatus, stream unsafe.Pointer) error {
	if rc := C.msh_schedule_sequential_fit_device(x.c, C.int32_t(p), (*C.int8_t)(dPodDigit), (*C.uint8_t)(dPodTol), C.int32_t(nres),
		(*C.int64_t)(dReq), C.int32_t(maxPodsPerNode), (*C.int32_t)(dIdx), (*C.int64_t)(dScore), (*C.int32_t)(dStatus), stream); rc != C.MSH_OK {
		return x.lastErr("msh_schedule_sequential_fit_device", rc)
	}
	return nil
}

// ResourceScore is the resource-aware score of ScheduleSequentialFit (msh_resource_score).
type ResourceScore int32

const (
	ResourceScoreNone           ResourceScore = C.MSH_RESOURCE_SCORE_NONE            // NodeNumber alone scores (the default)
	ResourceScoreLeastAllocated ResourceScore = C.MSH_RESOURCE_SCORE_LEAST_ALLOCATED // NodeResourcesLeastAllocated: spread
	ResourceScoreMostAllocated  ResourceScore = C.MSH_RESOURCE_SCORE_MOST_ALLOCATED  // NodeResourcesMostAllocated: pack
)

// SetResourceScore adds weight x the LeastAllocated / MostAllocated score of every feasible node to the totals of
// ScheduleSequentialFit and its device form; resWeights holds one weight in [0, 100] per resource of the table (0:
// fitted but not scored). Every other call ignores the setting, and it survives UploadNodes. Amounts must then stay
// within 2^55. The library substitutes no defaults for a pod that requests nothing.
func (x *Ctx) SetResourceScore(mode ResourceScore, weight int64, resWeights []int32) error {
	w := make([]C.int32_t, len(resWeights))
	for i, v := range resWeights {
		w[i] = C.int32_t(v)
	}
	if rc := C.msh_set_resource_score(x.c, C.int32_t(mode), C.int64_t(weight), C.int32_t(len(w)), ptrI32(w)); rc != C.MSH_OK {
		return x.lastErr("msh_set_resource_score", rc)
	}
	return nil
}

// ResourceScore returns the mode, the plugin weight and the resource weights the setting holds.
func (x *Ctx) ResourceScore() (mode ResourceScore, weight int64, resWeights []int32, err error) {
	var m, nr C.int32_t
	var wt C.int64_t
	w := make([]C.int32_t, int(C.MSH_MAX_RESOURCES))
	if rc := C.msh_get_resource_score(x.c, &m, &wt, &nr, ptrI32(w)); rc != C.MSH_OK {
		return ResourceScoreNone, 0, nil, x.lastErr("msh_get_resource_score", rc)
	}
	for i := 0; i < int(nr); i++ {
		resWeights = append(resWeights, int32(w[i]))
	}
	return ResourceScore(m), int64(wt), resWeights, nil
}

// SeqFitMaxNodes returns the largest table ScheduleSequentialFit takes with nres resources, without or with a
// resource score.
func (x *Ctx) SeqFitMaxNodes(nres int, scored bool) (int, error) {
	var out, sc C.int32_t
	if scored {
		sc = 1
	}
	if rc := C.msh_seq_fit_max_nodes(x.c, C.int32_t(nres), sc, &out); rc != C.MSH_OK {
		return 0, x.lastErr("msh_seq_fit_max_nodes", rc)
	}
	return int(out), nil
}

// ---- static node filters for sequential mode: per-class node masks ----
//
// nodeSelector, required NodeAffinity, TaintToleration (NoSchedule / NoExecute) and NodeName depend only on the
// pod's spec and the node's name, labels and taints. The caller groups the pods into at most MaxPodClasses classes of
// identical constraints, evaluates each class against each node once (upstream's own helpers do that in Go:
// nodeaffinity.GetRequiredNodeAffinity(pod).Match(node), v1helper.FindMatchingUntoleratedTaint) and uploads one
// uint64 per node in List order: bit c is set if the node admits pods of class c. ScheduleSequentialClasses is
// msh_schedule_sequential_spread_scored's contract with a class per pod (-1: none); group and class may be nil
// (no pod has a group / a class; nil groups need no zone column). UploadNodes drops the column; UpdateNodes keeps
// it; every other call ignores it. Like the rest of this package these calls have not been compiled (go/README.md).

// MaxPodClasses is MSH_MAX_POD_CLASSES.
const MaxPodClasses = int(C.MSH_MAX_POD_CLASSES)

func toU64(v []uint64) *C.uint64_t {
	if len(v) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&v[0]))
}

func toI32(v []int32) []C.int32_t {
	c := make([]C.int32_t, len(v))
	for i, x := range v {
		c[i] = C.int32_t(x)
	}
	return c
}

// UploadNodeClassBits sets the class column for nClasses classes (1..MaxPodClasses; no bit at or above nClasses).
func (x *Ctx) UploadNodeClassBits(nClasses int, bits []uint64) error {
	if rc := C.msh_upload_node_class_bits(x.c, C.int32_t(len(bits)), C.int32_t(nClasses), toU64(bits)); rc != C.MSH_OK {
		return x.lastErr("msh_upload_node_class_bits", rc)
	}
	return nil
}

// PatchNodeClassBits replaces the whole words of the nodes at idx (distinct List-order indices); nothing is rebuilt.
func (x *Ctx) PatchNodeClassBits(idx []int32, bits []uint64) error {
	if len(idx) != len(bits) {
		return errors.New("gpusched: idx / bits length mismatch")
	}
	if rc := C.msh_patch_node_class_bits(x.c, C.int32_t(len(idx)), ptrI32(toI32(idx)), toU64(bits)); rc != C.MSH_OK {
		return x.lastErr("msh_patch_node_class_bits", rc)
	}
	return nil
}

// ClearNodeClassBits goes back to "no column".
func (x *Ctx) ClearNodeClassBits() error {
	if rc := C.msh_clear_node_class_bits(x.c); rc != C.MSH_OK {
		return x.lastErr("msh_clear_node_class_bits", rc)
	}
	return nil
}

// NodeClassBits returns the number of classes and the column (n words, the uploaded node count), or 0 and nil when
// none is present.
func (x *Ctx) NodeClassBits(n int) (nClasses int, bits []uint64, err error) {
	var present, nc C.int32_t
	out := make([]uint64, n)
	if rc := C.msh_node_class_bits(x.c, &nc, toU64(out), &present); rc != C.MSH_OK {
		return 0, nil, x.lastErr("msh_node_class_bits", rc)
	}
	if present == 0 {
		return 0, nil, nil
	}
	return int(nc), out, nil
}

// SeqClassesMaxNodes returns the largest table ScheduleSequentialClasses takes with nres resources as the ctx is
// set now: the scored limits with a resource score, the topology-spread limits without.
func (x *Ctx) SeqClassesMaxNodes(nres int) (int, error) {
	var out C.int32_t
	if rc := C.msh_seq_classes_max_nodes(x.c, C.int32_t(nres), &out); rc != C.MSH_OK {
		return 0, x.lastErr("msh_seq_classes_max_nodes", rc)
	}
	return int(out), nil
}

// ScheduleSequentialClasses is ScheduleSequentialFit with a spread group and a class per pod (nil: none has one);
// req holds nres*len(pods) values (req[r*len(pods)+j]), nres may be 0 without a resource score.
func (x *Ctx) ScheduleSequentialClasses(pods []*v1.Pod, b *HostBatch, group, class []int32, nres int, req []int64,
	maxPodsPerNode int32) ([]Result, error) {
	if !x.hasNodes {
		return nil, errors.New("gpusched: UploadNodes has not been called")
	}
	p := len(pods)
	if len(req) != nres*p || (group != nil && len(group) != p) || (class != nil && len(class) != p) {
		return nil, errors.New("gpusched: req holds nres*len(pods) values, group and class len(pods)")
	}
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	if rc := C.msh_schedule_sequential_classes(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), ptrI32(toI32(group)),
		ptrI32(toI32(class)), C.int32_t(nres), ptrI64(toI64(req)), C.int32_t(maxPodsPerNode), ptrI32(b.idx[:p]),
		ptrI64(b.score[:p]), ptrI32(b.status[:p]), nil, nil); rc != C.MSH_OK {
		return nil, x.lastErr("msh_schedule_sequential_classes", rc)
	}
	return x.results(b), nil
}

// ScheduleSequentialClassesDevice is the asynchronous form over device pointers
// (msh_schedule_sequential_classes_device); dGroup and dClass may be nil, and nothing is validated by the library: a
// group outside [0, G) is an ungrouped pod, a class outside [0, C) a pod without one.
func (x *Ctx) ScheduleSequentialClassesDevice(p int, dPodDigit, dPodTol, dGroup, dClass unsafe.Pointer, nres int,
	dReq unsafe.Pointer, maxPodsPerNode int32, dIdx, dScore, dStatus, stream unsafe.Pointer) error {
	if rc := C.msh_schedule_sequential_classes_device(x.c, C.int32_t(p), (*C.int8_t)(dPodDigit), (*C.uint8_t)(dPodTol),
		(*C.int32_t)(dGroup), (*C.int32_t)(dClass), C.int32_t(nres), (*C.int64_t)(dReq), C.int32_t(maxPodsPerNode),
		(*C.int32_t)(dIdx), (*C.int64_t)(dScore), (*C.int32_t)(dStatus), stream); rc != C.MSH_OK {
		return x.lastErr("msh_schedule_sequential_classes_device", rc)
	}
	return nil
}

// ---- preferred node affinity and PreferNoSchedule scores (ABI v8, additive) ----
//
// Per (pod class, node) the caller gives A, the summed weights of the class's matching preferred node affinity
// terms, and T, the number of the node's PreferNoSchedule taints the class does not tolerate; the library
// normalises both per pod over its feasible nodes and adds wAffinity*na + wTaint*nt to the total
// (include/minisched_hip.h, "Preferred node affinity and PreferNoSchedule scores").

func toU16(v []uint16) *C.uint16_t {
	if len(v) == 0 {
		return nil
	}
	return (*C.uint16_t)(unsafe.Pointer(&v[0]))
}

// UploadNodeClassPrefs sets the preference column for nClasses classes over n nodes: affinity and taints hold
// nClasses*n values each, class-major in List order; either may be nil (all zero).
func (x *Ctx) UploadNodeClassPrefs(n, nClasses int, affinity, taints []uint16) error {
	if (affinity != nil && len(affinity) != n*nClasses) || (taints != nil && len(taints) != n*nClasses) {
		return errors.New("gpusched: affinity and taints hold nClasses*n values")
	}
	if rc := C.msh_upload_node_class_prefs(x.c, C.int32_t(n), C.int32_t(nClasses), toU16(affinity), toU16(taints)); rc != C.MSH_OK {
		return x.lastErr("msh_upload_node_class_prefs", rc)
	}
	return nil
}

// PatchNodeClassPrefs replaces the values of the nodes at idx for every class: nClasses*len(idx) values each,
// class-major; a nil slice writes zeros.
func (x *Ctx) PatchNodeClassPrefs(idx []int32, affinity, taints []uint16) error {
	if rc := C.msh_patch_node_class_prefs(x.c, C.int32_t(len(idx)), ptrI32(toI32(idx)), toU16(affinity), toU16(taints)); rc != C.MSH_OK {
		return x.lastErr("msh_patch_node_class_prefs", rc)
	}
	return nil
}

// ClearNodeClassPrefs goes back to "no column".
func (x *Ctx) ClearNodeClassPrefs() error {
	if rc := C.msh_clear_node_class_prefs(x.c); rc != C.MSH_OK {
		return x.lastErr("msh_clear_node_class_prefs", rc)
	}
	return nil
}

// NodeClassPrefs returns the number of classes and the two columns (nClasses*n values each, n the uploaded node
// count), or 0 and nil when none is present.
func (x *Ctx) NodeClassPrefs(n int) (nClasses int, affinity, taints []uint16, err error) {
	var present, nc C.int32_t
	if rc := C.msh_node_class_prefs(x.c, &nc, nil, nil, &present); rc != C.MSH_OK {
		return 0, nil, nil, x.lastErr("msh_node_class_prefs", rc)
	}
	if present == 0 {
		return 0, nil, nil, nil
	}
	affinity, taints = make([]uint16, int(nc)*n), make([]uint16, int(nc)*n)
	if rc := C.msh_node_class_prefs(x.c, &nc, toU16(affinity), toU16(taints), &present); rc != C.MSH_OK {
		return 0, nil, nil, x.lastErr("msh_node_class_prefs", rc)
	}
	return int(nc), affinity, taints, nil
}

// SetPreferenceWeights sets the two plugin weights, each in [0, 100]; 0 / 0 (the default) turns the scores off.
func (x *Ctx) SetPreferenceWeights(wAffinity, wTaint int) error {
	if rc := C.msh_set_preference_weights(x.c, C.int32_t(wAffinity), C.int32_t(wTaint)); rc != C.MSH_OK {
		return x.lastErr("msh_set_preference_weights", rc)
	}
	return nil
}

// PreferenceWeights returns the two plugin weights.
func (x *Ctx) PreferenceWeights() (wAffinity, wTaint int, err error) {
	var a, t C.int32_t
	if rc := C.msh_preference_weights(x.c, &a, &t); rc != C.MSH_OK {
		return 0, 0, x.lastErr("msh_preference_weights", rc)
	}
	return int(a), int(t), nil
}

// SeqPrefsMaxNodes returns the largest table ScheduleSequentialPrefs takes with nres resources.
func (x *Ctx) SeqPrefsMaxNodes(nres int) (int, error) {
	var out C.int32_t
	if rc := C.msh_seq_prefs_max_nodes(x.c, C.int32_t(nres), &out); rc != C.MSH_OK {
		return 0, x.lastErr("msh_seq_prefs_max_nodes", rc)
	}
	return int(out), nil
}

// ScheduleSequentialPrefs is ScheduleSequentialClasses with the two preference scores added to every feasible
// node's total; with both weights 0 it is ScheduleSequentialClasses.
func (x *Ctx) ScheduleSequentialPrefs(pods []*v1.Pod, b *HostBatch, group, class []int32, nres int, req []int64,
	maxPodsPerNode int32) ([]Result, error) {
	if !x.hasNodes {
		return nil, errors.New("gpusched: UploadNodes has not been called")
	}
	p := len(pods)
	if len(req) != nres*p || (group != nil && len(group) != p) || (class != nil && len(class) != p) {
		return nil, errors.New("gpusched: req holds nres*len(pods) values, group and class len(pods)")
	}
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	if rc := C.msh_schedule_sequential_prefs(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), ptrI32(toI32(group)),
		ptrI32(toI32(class)), C.int32_t(nres), ptrI64(toI64(req)), C.int32_t(maxPodsPerNode), ptrI32(b.idx[:p]),
		ptrI64(b.score[:p]), ptrI32(b.status[:p]), nil, nil); rc != C.MSH_OK {
		return nil, x.lastErr("msh_schedule_sequential_prefs", rc)
	}
	return x.results(b), nil
}

// ScheduleSequentialPrefsDevice is the asynchronous form over device pointers (msh_schedule_sequential_prefs_device);
// as ScheduleSequentialClassesDevice.
func (x *Ctx) ScheduleSequentialPrefsDevice(p int, dPodDigit, dPodTol, dGroup, dClass unsafe.Pointer, nres int,
	dReq unsafe.Pointer, maxPodsPerNode int32, dIdx, dScore, dStatus, stream unsafe.Pointer) error {
	if rc := C.msh_schedule_sequential_prefs_device(x.c, C.int32_t(p), (*C.int8_t)(dPodDigit), (*C.uint8_t)(dPodTol),
		(*C.int32_t)(dGroup), (*C.int32_t)(dClass), C.int32_t(nres), (*C.int64_t)(dReq), C.int32_t(maxPodsPerNode),
		(*C.int32_t)(dIdx), (*C.int64_t)(dScore), (*C.int32_t)(dStatus), stream); rc != C.MSH_OK {
		return x.lastErr("msh_schedule_sequential_prefs_device", rc)
	}
	return nil
}

// Spread group modes (msh_set_spread_group_modes).
const (
	SpreadDoNotSchedule  uint8 = C.MSH_SPREAD_DO_NOT_SCHEDULE
	SpreadScheduleAnyway uint8 = C.MSH_SPREAD_SCHEDULE_ANYWAY
)

// SetSpreadGroupModes gives each spread group its mode; len(modes) must be the current group count.
func (x *Ctx) SetSpreadGroupModes(modes []uint8) error {
	cm := make([]C.uint8_t, len(modes))
	for i, m := range modes {
		cm[i] = C.uint8_t(m)
	}
	if rc := C.msh_set_spread_group_modes(x.c, C.int32_t(len(modes)), ptrU8(cm)); rc != C.MSH_OK {
		return x.lastErr("msh_set_spread_group_modes", rc)
	}
	return nil
}

// SpreadGroupModes returns the groups' modes, one per group.
func (x *Ctx) SpreadGroupModes() ([]uint8, error) {
	var g C.int32_t
	if rc := C.msh_get_spread_group_modes(x.c, &g, nil); rc != C.MSH_OK {
		return nil, x.lastErr("msh_get_spread_group_modes", rc)
	}
	cm := make([]C.uint8_t, int(g))
	if rc := C.msh_get_spread_group_modes(x.c, &g, ptrU8(cm)); rc != C.MSH_OK {
		return nil, x.lastErr("msh_get_spread_group_modes", rc)
	}
	modes := make([]uint8, len(cm))
	for i, m := range cm {
		modes[i] = uint8(m)
	}
	return modes, nil
}

// SetSpreadScoreWeight sets the soft spread score's plugin weight, in [0, 100]; 0 is the default.
func (x *Ctx) SetSpreadScoreWeight(w int) error {
	if rc := C.msh_set_spread_score_weight(x.c, C.int32_t(w)); rc != C.MSH_OK {
		return x.lastErr("msh_set_spread_score_weight", rc)
	}
	return nil
}

// SpreadScoreWeight returns the soft spread score's plugin weight.
func (x *Ctx) SpreadScoreWeight() (int, error) {
	var w C.int32_t
	if rc := C.msh_spread_score_weight(x.c, &w); rc != C.MSH_OK {
		return 0, x.lastErr("msh_spread_score_weight", rc)
	}
	return int(w), nil
}

// SeqSoftMaxNodes returns the largest table ScheduleSequentialSoft takes with nres resources.
func (x *Ctx) SeqSoftMaxNodes(nres int) (int, error) {
	var out C.int32_t
	if rc := C.msh_seq_soft_max_nodes(x.c, C.int32_t(nres), &out); rc != C.MSH_OK {
		return 0, x.lastErr("msh_seq_soft_max_nodes", rc)
	}
	return int(out), nil
}

// ScheduleSequentialSoft is ScheduleSequentialPrefs, except that a pod of a SpreadScheduleAnyway group passes no
// spread filter and gets the spread score instead; with no such group it is ScheduleSequentialPrefs.
func (x *Ctx) ScheduleSequentialSoft(pods []*v1.Pod, b *HostBatch, group, class []int32, nres int, req []int64,
	maxPodsPerNode int32) ([]Result, error) {
	if !x.hasNodes {
		return nil, errors.New("gpusched: UploadNodes has not been called")
	}
	p := len(pods)
	if len(req) != nres*p || (group != nil && len(group) != p) || (class != nil && len(class) != p) {
		return nil, errors.New("gpusched: req holds nres*len(pods) values, group and class len(pods)")
	}
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	if rc := C.msh_schedule_sequential_soft(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), ptrI32(toI32(group)),
		ptrI32(toI32(class)), C.int32_t(nres), ptrI64(toI64(req)), C.int32_t(maxPodsPerNode), ptrI32(b.idx[:p]),
		ptrI64(b.score[:p]), ptrI32(b.status[:p]), nil, nil); rc != C.MSH_OK {
		return nil, x.lastErr("msh_schedule_sequential_soft", rc)
	}
	return x.results(b), nil
}

// ScheduleSequentialSoftDevice is the asynchronous form over device pointers (msh_schedule_sequential_soft_device);
// as ScheduleSequentialPrefsDevice.
func (x *Ctx) ScheduleSequentialSoftDevice(p int, dPodDigit, dPodTol, dGroup, dClass unsafe.Pointer, nres int,
	dReq unsafe.Pointer, maxPodsPerNode int32, dIdx, dScore, dStatus, stream unsafe.Pointer) error {
	if rc := C.msh_schedule_sequential_soft_device(x.c, C.int32_t(p), (*C.int8_t)(dPodDigit), (*C.uint8_t)(dPodTol),
		(*C.int32_t)(dGroup), (*C.int32_t)(dClass), C.int32_t(nres), (*C.int64_t)(dReq), C.int32_t(maxPodsPerNode),
		(*C.int32_t)(dIdx), (*C.int64_t)(dScore), (*C.int32_t)(dStatus), stream); rc != C.MSH_OK {
		return x.lastErr("msh_schedule_sequential_soft_device", rc)
	}
	return nil
}

// SetBalancedScore sets NodeResourcesBalancedAllocation's plugin weight, in [0, 100]; 0 is the default.
func (x *Ctx) SetBalancedScore(w int) error {
	if rc := C.msh_set_balanced_score(x.c, C.int32_t(w)); rc != C.MSH_OK {
		return x.lastErr("msh_set_balanced_score", rc)
	}
	return nil
}

// BalancedScore returns the balanced-allocation score's plugin weight.
func (x *Ctx) BalancedScore() (int, error) {
	var w C.int32_t
	if rc := C.msh_balanced_score(x.c, &w); rc != C.MSH_OK {
		return 0, x.lastErr("msh_balanced_score", rc)
	}
	return int(w), nil
}

// SeqBalancedMaxNodes returns the largest table ScheduleSequentialBalanced takes with nres resources.
func (x *Ctx) SeqBalancedMaxNodes(nres int) (int, error) {
	var out C.int32_t
	if rc := C.msh_seq_balanced_max_nodes(x.c, C.int32_t(nres), &out); rc != C.MSH_OK {
		return 0, x.lastErr("msh_seq_balanced_max_nodes", rc)
	}
	return int(out), nil
}

// ScheduleSequentialBalanced is ScheduleSequentialSoft with the balanced-allocation score of the table's first two
// resources, times its weight, added to every feasible node's total; with the weight 0 it is ScheduleSequentialSoft.
func (x *Ctx) ScheduleSequentialBalanced(pods []*v1.Pod, b *HostBatch, group, class []int32, nres int, req []int64,
	maxPodsPerNode int32) ([]Result, error) {
	if !x.hasNodes {
		return nil, errors.New("gpusched: UploadNodes has not been called")
	}
	p := len(pods)
	if len(req) != nres*p || (group != nil && len(group) != p) || (class != nil && len(class) != p) {
		return nil, errors.New("gpusched: req holds nres*len(pods) values, group and class len(pods)")
	}
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	if rc := C.msh_schedule_sequential_balanced(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), ptrI32(toI32(group)),
		ptrI32(toI32(class)), C.int32_t(nres), ptrI64(toI64(req)), C.int32_t(maxPodsPerNode), ptrI32(b.idx[:p]),
		ptrI64(b.score[:p]), ptrI32(b.status[:p]), nil, nil); rc != C.MSH_OK {
		return nil, x.lastErr("msh_schedule_sequential_balanced", rc)
	}
	return x.results(b), nil
}

// ScheduleSequentialBalancedDevice is the asynchronous form over device pointers
// (msh_schedule_sequential_balanced_device); as ScheduleSequentialSoftDevice.
func (x *Ctx) ScheduleSequentialBalancedDevice(p int, dPodDigit, dPodTol, dGroup, dClass unsafe.Pointer, nres int,
	dReq unsafe.Pointer, maxPodsPerNode int32, dIdx, dScore, dStatus, stream unsafe.Pointer) error {
	if rc := C.msh_schedule_sequential_balanced_device(x.c, C.int32_t(p), (*C.int8_t)(dPodDigit), (*C.uint8_t)(dPodTol),
		(*C.int32_t)(dGroup), (*C.int32_t)(dClass), C.int32_t(nres), (*C.int64_t)(dReq), C.int32_t(maxPodsPerNode),
		(*C.int32_t)(dIdx), (*C.int64_t)(dScore), (*C.int32_t)(dStatus), stream); rc != C.MSH_OK {
		return x.lastErr("msh_schedule_sequential_balanced_device", rc)
	}
	return nil
}

// ---- required inter-pod affinity and anti-affinity ----

// Topologies of an inter-pod affinity term (MSH_TOPOLOGY_*), and the limits of a ctx.
const (
	TopologyHostname = 0
	TopologyZone     = 1
	MaxAffinityTerms = 32
	MaxPodProfiles   = 64
)

func toU32(v []uint32) *C.uint32_t {
	if len(v) == 0 {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&v[0]))
}

// SetPodAffinityTerms sets the terms' topologies (at most MaxAffinityTerms), drops the profiles and zeroes the state;
// an empty slice is "no terms".
func (x *Ctx) SetPodAffinityTerms(topo []uint8) error {
	var p *C.uint8_t
	if len(topo) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&topo[0]))
	}
	if rc := C.msh_set_pod_affinity_terms(x.c, C.int32_t(len(topo)), p); rc != C.MSH_OK {
		return x.lastErr("msh_set_pod_affinity_terms", rc)
	}
	return nil
}

// PodAffinityTerms returns the terms' topologies.
func (x *Ctx) PodAffinityTerms() ([]uint8, error) {
	var t C.int32_t
	out := make([]uint8, MaxAffinityTerms)
	if rc := C.msh_get_pod_affinity_terms(x.c, &t, (*C.uint8_t)(unsafe.Pointer(&out[0]))); rc != C.MSH_OK {
		return nil, x.lastErr("msh_get_pod_affinity_terms", rc)
	}
	return out[:int(t)], nil
}

// SetPodProfiles sets the pod profiles (at most MaxPodProfiles): per profile the terms a pod of it satisfies, its own
// required anti-affinity terms, and its one required affinity term (-1: none).
func (x *Ctx) SetPodProfiles(match, anti []uint32, aff []int32) error {
	if len(match) != len(anti) || len(match) != len(aff) {
		return errors.New("gpusched: match / anti / aff length mismatch")
	}
	if rc := C.msh_set_pod_profiles(x.c, C.int32_t(len(match)), toU32(match), toU32(anti), ptrI32(toI32(aff))); rc != C.MSH_OK {
		return x.lastErr("msh_set_pod_profiles", rc)
	}
	return nil
}

// PodProfiles returns the profiles (match, anti, aff).
func (x *Ctx) PodProfiles() (match, anti []uint32, aff []int32, err error) {
	var q C.int32_t
	match, anti = make([]uint32, MaxPodProfiles), make([]uint32, MaxPodProfiles)
	a := make([]C.int32_t, MaxPodProfiles)
	if rc := C.msh_get_pod_profiles(x.c, &q, toU32(match), toU32(anti), &a[0]); rc != C.MSH_OK {
		return nil, nil, nil, x.lastErr("msh_get_pod_profiles", rc)
	}
	aff = make([]int32, int(q))
	for i := range aff {
		aff[i] = int32(a[i])
	}
	return match[:int(q)], anti[:int(q)], aff, nil
}

// UploadPodAffinityState sets the per-node state: present (the OR of the match bits of the pods a node holds) and repel
// (the OR of their anti-affinity terms), one word per uploaded node each; a nil slice is zeros. UploadNodes zeroes it.
func (x *Ctx) UploadPodAffinityState(n int, present, repel []uint32) error {
	if (present != nil && len(present) != n) || (repel != nil && len(repel) != n) {
		return errors.New("gpusched: one state word per uploaded node")
	}
	if rc := C.msh_upload_pod_affinity_state(x.c, C.int32_t(n), toU32(present), toU32(repel)); rc != C.MSH_OK {
		return x.lastErr("msh_upload_pod_affinity_state", rc)
	}
	return nil
}

// PatchPodAffinityState replaces the whole words of the nodes at idx (distinct List-order indices); a nil slice writes
// zeros. Pods that were bound before the node snapshot are entered this way.
func (x *Ctx) PatchPodAffinityState(idx []int32, present, repel []uint32) error {
	if (present != nil && len(present) != len(idx)) || (repel != nil && len(repel) != len(idx)) {
		return errors.New("gpusched: idx / state length mismatch")
	}
	if rc := C.msh_patch_pod_affinity_state(x.c, C.int32_t(len(idx)), ptrI32(toI32(idx)), toU32(present), toU32(repel)); rc != C.MSH_OK {
		return x.lastErr("msh_patch_pod_affinity_state", rc)
	}
	return nil
}

// PodAffinityState reads the state of the n uploaded nodes back.
func (x *Ctx) PodAffinityState(n int) (present, repel []uint32, err error) {
	present, repel = make([]uint32, n), make([]uint32, n)
	if rc := C.msh_pod_affinity_state(x.c, toU32(present), toU32(repel)); rc != C.MSH_OK {
		return nil, nil, x.lastErr("msh_pod_affinity_state", rc)
	}
	return present, repel, nil
}

// SeqPodAffinityMaxNodes returns the largest table ScheduleSequentialPodAffinity takes with nres resources.
func (x *Ctx) SeqPodAffinityMaxNodes(nres int) (int, error) {
	var out C.int32_t
	if rc := C.msh_seq_podaffinity_max_nodes(x.c, C.int32_t(nres), &out); rc != C.MSH_OK {
		return 0, x.lastErr("msh_seq_podaffinity_max_nodes", rc)
	}
	return int(out), nil
}

// ScheduleSequentialPodAffinity is ScheduleSequentialBalanced with a profile per pod (-1: none): the required
// inter-pod affinity and anti-affinity filter narrows the feasible set, and each placement is committed to the state
// before the next pod. A nil profile slice is ScheduleSequentialBalanced.
func (x *Ctx) ScheduleSequentialPodAffinity(pods []*v1.Pod, b *HostBatch, group, class, profile []int32, nres int,
	req []int64, maxPodsPerNode int32) ([]Result, error) {
	if !x.hasNodes {
		return nil, errors.New("gpusched: UploadNodes has not been called")
	}
	p := len(pods)
	if len(req) != nres*p || (group != nil && len(group) != p) || (class != nil && len(class) != p) ||
		(profile != nil && len(profile) != p) {
		return nil, errors.New("gpusched: req holds nres*len(pods) values, group, class and profile len(pods)")
	}
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	if rc := C.msh_schedule_sequential_podaffinity(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), ptrI32(toI32(group)),
		ptrI32(toI32(class)), ptrI32(toI32(profile)), C.int32_t(nres), ptrI64(toI64(req)), C.int32_t(maxPodsPerNode),
		ptrI32(b.idx[:p]), ptrI64(b.score[:p]), ptrI32(b.status[:p]), nil, nil); rc != C.MSH_OK {
		return nil, x.lastErr("msh_schedule_sequential_podaffinity", rc)
	}
	return x.results(b), nil
}

// ScheduleSequentialPodAffinityDevice is the asynchronous form over device pointers
// (msh_schedule_sequential_podaffinity_device); a profile outside [0, Q) is a pod without one.
func (x *Ctx) ScheduleSequentialPodAffinityDevice(p int, dPodDigit, dPodTol, dGroup, dClass, dProfile unsafe.Pointer,
	nres int, dReq unsafe.Pointer, maxPodsPerNode int32, dIdx, dScore, dStatus, stream unsafe.Pointer) error {
	if rc := C.msh_schedule_sequential_podaffinity_device(x.c, C.int32_t(p), (*C.int8_t)(dPodDigit), (*C.uint8_t)(dPodTol),
		(*C.int32_t)(dGroup), (*C.int32_t)(dClass), (*C.int32_t)(dProfile), C.int32_t(nres), (*C.int64_t)(dReq),
		C.int32_t(maxPodsPerNode), (*C.int32_t)(dIdx), (*C.int64_t)(dScore), (*C.int32_t)(dStatus), stream); rc != C.MSH_OK {
		return x.lastErr("msh_schedule_sequential_podaffinity_device", rc)
	}
	return nil
}

// ---- node sharding (ABI v8): the node table split over GPUs, the cross-shard merge inside the library ----
//
// The reference's selectHost keeps the first maximum of the whole List-order node list
// (minisched.go:304-325). Split into contiguous slices, each shard finds its own first maximum per pod,
// and the library merges them back into the global one: in one process over several devices (Group), or
// one process per GPU over an RCCL communicator (Ctx.InitComm + ScheduleNodeShard).

// sortedNodes is the List order of nodes (byte-sorted names, the apiserver's etcd key order).
func sortedNodes(nodes []v1.Node) []*v1.Node {
	sorted := make([]*v1.Node, len(nodes))
	for i := range nodes {
		sorted[i] = &nodes[i]
	}
	sort.Slice(sorted, func(a, b int) bool { return sorted[a].Name < sorted[b].Name })
	return sorted
}

// shardRange is the contiguous slice [lo, hi) of n List positions that shard k of w holds.
func shardRange(n, w, k int) (int, int) { return n * k / w, n * (k + 1) / w }

// uploadSlice uploads List positions [lo, hi) of sorted as x's table.
func (x *Ctx) uploadSlice(sorted []*v1.Node, lo, hi int) error {
	uns := make([]C.uint8_t, hi-lo)
	dig := make([]C.int8_t, hi-lo)
	for i, n := range sorted[lo:hi] {
		if n.Spec.Unschedulable {
			uns[i] = 1
		}
		dig[i] = C.int8_t(suffixDigit(n.Name))
	}
	if rc := C.msh_upload_nodes(x.c, C.int32_t(hi-lo), ptrU8(uns), ptrI8(dig)); rc != C.MSH_OK {
		return x.lastErr("msh_upload_nodes", rc)
	}
	x.hasNodes = true
	return nil
}

// Group is one scheduler process driving several GPUs (msh_group_*): shard k (a Ctx on devices[k])
// holds the k-th contiguous slice of the List order; msh_group_schedule_batch runs every shard's kernel
// on its own device and merges on devices[0], reading the shards' per-pod results over xGMI.
type Group struct {
	g       *C.msh_group
	shards  []*Ctx
	byIndex []*v1.Node // global List order
}

// NewGroup creates one shard Ctx per device (the same plugin lists on each) and the group over them.
func NewGroup(devices []int, filters []framework.FilterPlugin, preScores []framework.PreScorePlugin,
	scores []ScoreConfig) (*Group, error) {
	if len(devices) < 1 || len(devices) > C.MSH_GROUP_MAX_SHARDS {
		return nil, fmt.Errorf("gpusched: 1..%d devices", int(C.MSH_GROUP_MAX_SHARDS))
	}
	gr := &Group{}
	for _, d := range devices {
		x, err := New(d, filters, preScores, scores)
		if err != nil {
			gr.Close()
			return nil, err
		}
		gr.shards = append(gr.shards, x)
	}
	cs := make([]*C.msh_ctx, len(gr.shards)) // C memory holds no Go pointer: the handles are C pointers
	for k, x := range gr.shards {
		cs[k] = x.c
	}
	if rc := C.msh_group_create(&cs[0], C.int32_t(len(cs)), &gr.g); rc != C.MSH_OK {
		err := fmt.Errorf("msh_group_create: %d: %s", int(rc), C.GoString(C.msh_group_last_error(nil)))
		gr.Close()
		return nil, err
	}
	runtime.SetFinalizer(gr, (*Group).Close)
	return gr, nil
}

// Close releases the group, then its shard contexts.
func (gr *Group) Close() {
	if gr.g != nil {
		C.msh_group_destroy(gr.g)
		gr.g = nil
	}
	for _, x := range gr.shards {
		x.Close()
	}
	gr.shards = nil
	runtime.SetFinalizer(gr, nil)
}

// UploadNodes puts the nodes in List order and uploads slice k to shard k (replacing minisched.go:40).
func (gr *Group) UploadNodes(nodes []v1.Node) error {
	sorted := sortedNodes(nodes)
	for k, x := range gr.shards {
		lo, hi := shardRange(len(sorted), len(gr.shards), k)
		if err := x.uploadSlice(sorted, lo, hi); err != nil {
			return err
		}
	}
	gr.byIndex = sorted
	return nil
}

// ScheduleBatch runs minisched.go:50-87 for every pod against the whole (sharded) table, synchronously.
func (gr *Group) ScheduleBatch(pods []*v1.Pod, b *HostBatch) ([]Result, error) {
	if gr.byIndex == nil {
		return nil, errors.New("gpusched: UploadNodes has not been called")
	}
	x := &Ctx{byIndex: gr.byIndex} // packing and decoding against the global List order
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	p := len(pods)
	if rc := C.msh_group_schedule_batch(gr.g, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), ptrI32(b.idx[:p]),
		ptrI64(b.score[:p]), ptrI32(b.status[:p])); rc != C.MSH_OK {
		return nil, fmt.Errorf("msh_group_schedule_batch: %d: %s", int(rc), C.GoString(C.msh_group_last_error(gr.g)))
	}
	return x.results(b), nil
}

// CommID makes the id of a new RCCL communicator (msh_comm_unique_id): rank 0 calls it and ships the
// bytes to every rank (over the scheduler's own channel).
func CommID() ([]byte, error) {
	buf := make([]byte, C.MSH_COMM_ID_BYTES)
	if rc := C.msh_comm_unique_id((*C.uint8_t)(unsafe.Pointer(&buf[0]))); rc != C.MSH_OK {
		return nil, fmt.Errorf("msh_comm_unique_id: %d", int(rc))
	}
	return buf, nil
}

// InitComm joins x to the communicator `id` as rank `rank` of `world` (one process per GPU); it returns
// once every rank has joined.
func (x *Ctx) InitComm(id []byte, world, rank int) error {
	if len(id) != C.MSH_COMM_ID_BYTES {
		return fmt.Errorf("gpusched: a comm id is %d bytes", int(C.MSH_COMM_ID_BYTES))
	}
	cid := C.CBytes(id) // C memory: the library reads it during the call
	defer C.free(cid)
	if rc := C.msh_comm_init(x.c, (*C.uint8_t)(cid), C.int32_t(world), C.int32_t(rank)); rc != C.MSH_OK {
		return x.lastErr("msh_comm_init", rc)
	}
	return nil
}

// UploadNodeShard keeps the whole List order for decoding (every rank's informer holds every node) and
// uploads this rank's slice; it returns the slice's global base for ScheduleNodeShard.
func (x *Ctx) UploadNodeShard(nodes []v1.Node, world, rank int) (int64, error) {
	sorted := sortedNodes(nodes)
	lo, hi := shardRange(len(sorted), world, rank)
	if err := x.uploadSlice(sorted, lo, hi); err != nil {
		return 0, err
	}
	x.byIndex = sorted
	return int64(lo), nil
}

// ScheduleNodeShard is ScheduleBatch over the table split across the communicator's ranks
// (msh_schedule_nodeshard): every rank calls it with the same pods and gets every pod's decision.
func (x *Ctx) ScheduleNodeShard(pods []*v1.Pod, b *HostBatch, nodeBase int64) ([]Result, error) {
	if !x.hasNodes {
		return nil, errors.New("gpusched: UploadNodeShard has not been called")
	}
	if err := x.pack(b, pods); err != nil {
		return nil, err
	}
	p := len(pods)
	if rc := C.msh_schedule_nodeshard(x.c, C.int32_t(p), ptrI8(b.pd[:p]), ptrU8(b.pt[:p]), C.int64_t(nodeBase),
		ptrI32(b.idx[:p]), ptrI64(b.score[:p]), ptrI32(b.status[:p])); rc != C.MSH_OK {
		return nil, x.lastErr("msh_schedule_nodeshard", rc)
	}
	return x.results(b), nil
}

// suffixDigit is strconv.Atoi(name[len(name)-1:]) (nodenumber.go:51-56, :81-87): only '0'..'9' parse.
func suffixDigit(name string) int {
	if name == "" {
		return -1
	}
	c := name[len(name)-1]
	if c >= '0' && c <= '9' {
		return int(c - '0')
	}
	return -1
}

// tolerates is v1helper.TolerationsTolerateTaint(tolerations, unschedulable taint), what upstream
// NodeUnschedulable.Filter (k8s.io/kubernetes v1.22.0) asks.
func tolerates(ts []v1.Toleration) bool {
	taint := &v1.Taint{Key: v1.TaintNodeUnschedulable, Effect: v1.TaintEffectNoSchedule}
	for i := range ts {
		if ts[i].ToleratesTaint(taint) {
			return true
		}
	}
	return false
}

func ptrI32(s []C.int32_t) *C.int32_t {
	if len(s) == 0 {
		return nil
	}
	return &s[0]
}

func ptrI64(s []C.int64_t) *C.int64_t {
	if len(s) == 0 {
		return nil
	}
	return &s[0]
}

func ptrU8(s []C.uint8_t) *C.uint8_t {
	if len(s) == 0 {
		return nil
	}
	return &s[0]
}

func ptrI8(s []C.int8_t) *C.int8_t {
	if len(s) == 0 {
		return nil
	}
	return &s[0]
}
